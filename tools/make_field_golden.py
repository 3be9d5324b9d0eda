"""Mints tests/golden/field_ref.npz from the reference's own GaussianModel (filters + extract_fields) on the CPU.

    python tools/make_field_golden.py --reference /path/to/Open-DiffusionGS

Needs the reference tree; run where it exists (the suite itself reads only the fixture).  gs_core.py is loaded by path with empty
stand-ins for the modules it imports but this code path never calls (cv2, plyfile, imageio, trimesh, matplotlib,
diffusionGS.utils.mesh_utils, the rasterizer binding) and a `kiui` whose `lo` does nothing.  Scenes: tests/field_util.py make_scene.
Per case the fixture holds the scene's digest (and, for the small cases, the raw inputs), the masks of apply_all_filters with the
pipeline's arguments (recorded from the reference's `filter` calls) and the surviving counts, mesh_center / mesh_scale and the
reference's fp32 occ: the whole field, or for the large case the blocks of a seeded sample."""
import argparse
import importlib.util
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import field_util as U  # noqa: E402


def load_reference(tree):
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    for name in ("cv2", "imageio", "trimesh", "matplotlib"):
        stub(name)
    stub("plyfile", PlyData=None, PlyElement=None)
    stub("diff_gaussian_rasterization", GaussianRasterizationSettings=None, GaussianRasterizer=None)
    stub("kiui", lo=lambda *a, **k: None)
    stub("diffusionGS").__path__ = []
    stub("diffusionGS.utils").__path__ = []
    stub("diffusionGS.utils.mesh_utils", decimate_mesh=None, clean_mesh=None)
    try:
        import einops  # noqa: F401
    except ImportError:
        stub("einops", rearrange=None)
    spec = importlib.util.spec_from_file_location("ref_gs_core", os.path.join(tree, "diffusionGS", "models", "gsrenderer", "gs_core.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=U.GOLDEN)
    args = ap.parse_args()
    ref = load_reference(args.reference)
    out = {}
    for name, (n, r, nb, seed, sampled) in U.FIXTURE_CASES.items():
        scene = U.make_scene(n, seed)
        pc = ref.GaussianModel(0).set_data(*(scene[k].clone() for k in ("xyz", "features", "scaling", "rotation", "opacity")))
        masks, plain = [], pc.filter
        pc.filter = lambda m: (masks.append(m.clone()), plain(m))[1]
        assert pc.apply_all_filters(**U.PIPELINE_FILTERS) is pc
        prune, crop = masks
        both = prune.clone()
        both[prune] = crop
        t0 = time.time()
        occ = pc.extract_fields(r, nb)
        print(f"{name}: reference extract_fields {time.time() - t0:.1f} s, kept {int(both.sum())} of {n}, max {float(occ.max()):.4g}")
        out[f"{name}/digest"] = np.array(U.scene_digest(scene))
        if n <= 4000:
            for k in ("xyz", "scaling", "rotation", "opacity"):
                out[f"{name}/{k}"] = scene[k].numpy()
        out[f"{name}/mask_prune"], out[f"{name}/mask_crop"], out[f"{name}/mask_all"] = prune.numpy(), crop.numpy(), both.numpy()
        out[f"{name}/counts"] = np.array([int(prune.sum()), int(both.sum())])
        out[f"{name}/mesh_center"], out[f"{name}/mesh_scale"] = pc.mesh_center.numpy(), np.array(pc.mesh_scale, dtype=np.float64)
        if sampled is None:
            out[f"{name}/occ"] = occ.numpy()
        else:
            blocks = U.sample_blocks(nb, sampled, seed)
            out[f"{name}/blocks"] = np.array(blocks, dtype=np.int32)
            out[f"{name}/occ"] = U.gather_blocks(occ, nb, blocks).numpy()
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
