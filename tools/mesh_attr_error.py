"""Measured error over bar of the mesh attributes (csrc/mesh_attr.hip) per case, and the bytes of the default field / mesh calls against
another build of the library.
    python tools/mesh_attr_error.py --device cpu                 the checks of tests/test_mesh_attr.py that go through the fp64 restatement
                                                                 (tests/mesh_attr_util.py) on the emulated build; writes the lines they
                                                                 print to profiles/mesh_attr_parity.txt.  Below 1 is inside the bar.
    python tools/mesh_attr_error.py --device cuda:0 --append     the same on the product library (there also the r64_nb16 scene), appended:
                                                                 the committed file is these two runs, in this order
    python tools/mesh_attr_error.py --parent-library PATH        needs a GPU.  extract_fields and extract_mesh() with default arguments on
                                                                 five scenes with this tree's library and with the one at PATH (the
                                                                 parent commit's field.hip: tools/ab_build.sh field.hip <parent>), byte
                                                                 for byte, with the SHA-256 of occ / vertices / faces; writes
                                                                 profiles/mesh_attr_parent_bytes.txt.  The r32_nb8 line is where the
                                                                 digests pinned in tests/test_mesh_attr_gpu.py come from.
    [--out FILE]"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def parent_bytes(args):
    import torch

    import field_util as U
    from dgs_amd import _native, consumers
    new, base = _native.lib(), _native.open_library(os.path.abspath(args.parent_library))
    lines = ["# extract_fields / extract_mesh() with default arguments: this tree's library against " + os.path.basename(args.parent_library) +
             " (tools/mesh_attr_error.py --parent-library) on " + torch.cuda.get_device_name(0),
             "# scene: SHA-256 of occ, vertices, faces with the parent's library; then whether this tree's library gives the same bytes"]
    same = True
    fixture = U.golden_scene("r32_nb8")[1]                                    # the scene the GPU test pins
    scenes = [("r32_nb8 fixture (filtered)", fixture, 32, 8)] + [(f"make_scene({n}, {seed}) R {r} nb {nb}", U.make_scene(n, seed), r, nb)
                                                                  for n, seed, r, nb in ((2000, 2, 40, 4), (20000, 3, 64, 16), (65536, 31, 128, 32), (262144, 21, 256, 64))]
    for name, scene, r, nb in scenes:
        pc = U.make_model(scene, "cuda:0")
        a, b = consumers.extract_fields(pc, r, nb, lib=base), consumers.extract_fields(pc, r, nb, lib=new)
        ma, mb = consumers.extract_mesh(pc, resolution=r, num_blocks=nb, lib=base), consumers.extract_mesh(pc, resolution=r, num_blocks=nb, lib=new)
        ok = torch.equal(a, b) and torch.equal(ma.vertices, mb.vertices) and torch.equal(ma.faces, mb.faces)
        same = same and ok
        lines.append(f"{name}: V {ma.vertices.shape[0]} F {ma.faces.shape[0]} occ {digest(a)} vertices {digest(ma.vertices)} faces {digest(ma.faces)}: "
                     + ("identical bytes" if ok else "DIFFERENT"))
        print(lines[-1], flush=True)
    with open(args.out or os.path.join(ROOT, "profiles", "mesh_attr_parent_bytes.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    if not same:
        raise SystemExit("mesh_attr_error.py: the two libraries differ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--parent-library", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.parent_library:
        return parent_bytes(args)
    import torch

    import test_mesh_attr as T
    dev = args.device
    if dev != "cpu" and not torch.cuda.is_available():
        raise SystemExit("mesh_attr_error.py: no GPU")
    T.check_trivial(dev)
    T.check_sphere(dev)
    T.check_crowded(dev)
    T.check_edges(dev)
    for name in ("r32_nb8", "r40_nb4"):
        for filtered in (False, True):
            T.check_fixture(dev, name, filtered)
    if dev != "cpu":
        T.check_fixture(dev, "r64_nb16", False)
    head = (f"# err / bar per output and case, tools/mesh_attr_error.py --device {dev} (bars: tests/mesh_attr_util.py; below 1 is inside the bar): "
            + ("the emulated build" if dev == "cpu" else "the product library on " + torch.cuda.get_device_name(0)))
    out = args.out or os.path.join(ROOT, "profiles", "mesh_attr_parity.txt")
    with open(out, "a" if args.append else "w") as f:
        f.write(head + "\n" + "\n".join(T.REPORT) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
