"""Forward-only consumers of the rasterizer: the turntable render and the 3DGS .ply wire format.

Mirrors diffusionGS/models/gsrenderer/gs_core.py:
    get_turntable_cameras                      :50-85
    render_turntable                           :1203-1219   (reference: one rasterizer call + ~15 camera ops + syncs PER VIEW;
                                                             here all views are one batched launch sequence of the HIP rasterizer)
    render_generic                             :1300-1316   (same, for caller-supplied cameras; [v, h, w, 3] uint8)
    GaussianModel.construct_dtypes / save_ply / load_ply   :578-760   (the layout 3DGS viewers read: x y z, red green blue,
                                                             f_dc_*, f_rest_* padded to SH degree 3, opacity, scale_*, rot_*)
    GaussianModel.extract_fields               :786-852     (reference: a host loop over num_blocks^3 blocks, ~15 torch ops and a
                                                             synchronisation each; here one C call, csrc/field.hip)
    GaussianModel.extract_mesh                 :855-860     (reference: occ to the host, `mcubes.marching_cubes`; here two C calls on
                                                             the device grid, csrc/mesh.hip, and a two-integer readback between them)
and of diffusionGS/utils/mesh_utils.py clean_mesh :119-125  (the two pymeshlab filters that remove small connected components; here
                                                             remove_small_components, csrc/mesh_clean.hip, a five-integer readback)
                                   decimate_mesh :44-85     (pymeshlab's quadric edge collapse, order-dependent; here its commented
                                                             alternative, vertex clustering, with an order-free definition:
                                                             cluster_vertices / decimate_mesh, csrc/mesh_decimate.hip)
                                   clean_mesh :133, decimate_mesh :71  (ms.apply_coord_taubin_smoothing(), the commented alternative
                                                             of their remeshing; here smooth_mesh, csrc/mesh_smooth.hip)
                                   clean_mesh :116-117, :127-130  (pymeshlab's duplicate-face, null-face, non-manifold edge and
                                                             non-manifold vertex filters; here their order-free form, repair_mesh and
                                                             the census mesh_topology, csrc/mesh_repair.hip)
The reference writes / reads the file through the `plyfile` package (binary_little_endian 1.0, one "vertex" element, scalar
properties in dtype order); that byte layout is restated here with numpy structured arrays -- no extra dependency.
"""
import ctypes
import math
import os

import numpy as np
import torch

C0 = 0.28209479177387814       # SH2RGB, gs_core.py (utils.sh_utils): rgb = sh * C0 + 0.5

_PLY_TYPES = {"f4": "float", "f2": None, "u1": "uchar"}


def get_turntable_cameras(hfov=50, num_views=8, w=384, h=384, radius=2.7, elevation=0, up_vector=np.array([0, 0, 1])):
    """gs_core.py:50-85.  -> (w, h, num_views, fxfycxcy [v, 4], c2w [v, 4, 4]) float64, OpenCV convention."""
    fx = w / (2 * np.tan(np.deg2rad(hfov) / 2.0))
    fxfycxcy = np.array([fx, fx, w / 2.0, h / 2.0]).reshape(1, 4).repeat(num_views, axis=0)
    c2ws = []
    for azim in np.linspace(0, 360, num_views, endpoint=False):
        elev, azim = np.deg2rad(elevation), np.deg2rad(azim)
        base = radius * np.cos(elev)
        cam_pos = np.array([base * np.cos(azim), base * np.sin(azim), radius * np.sin(elev)])
        forward = -cam_pos / np.linalg.norm(cam_pos)
        right = np.cross(forward, up_vector)
        right = right / np.linalg.norm(right)
        up = np.cross(right, forward)
        up = up / np.linalg.norm(up)
        c2w = np.eye(4)
        c2w[:3, :4] = np.concatenate((np.stack((right, -up, forward), axis=1), cam_pos[:, None]), axis=1)
        c2ws.append(c2w)
    return w, h, num_views, fxfycxcy, np.stack(c2ws, axis=0)


def render_turntable(pc, rendering_resolution=384, num_views=8, backend=None, return_aux=False):
    """gs_core.py:1203-1219: `pc` a GaussianModel -> uint8 image strip [h, v*w, 3].
    return_aux=True -> (strip, depth float32 [h, v*w], alpha float32 [h, v*w]) from the same render: un-normalised expected depth
    (divide by alpha for a mean depth) and accumulated opacity."""
    from .raster import default_backend
    w, h, v, fxfycxcy, c2w = get_turntable_cameras(h=rendering_resolution, w=rendering_resolution, num_views=num_views)
    dev = pc._xyz.device
    k = torch.from_numpy(fxfycxcy).float().to(dev)[None]
    c = torch.from_numpy(c2w).float().to(dev)[None]
    be = backend if backend is not None else default_backend()
    feats = pc.get_features.float()[None]
    r = be.render_views(pc._xyz.float()[None], feats, pc._scaling.float()[None], pc._rotation.float()[None], pc._opacity.float()[None],
                        h, w, c, k, **(dict(aux=True) if return_aux else {}))
    r, maps = (r[0][0], [m[0, :, 0].detach().cpu().numpy() for m in r[1:]]) if return_aux else (r[0], None)   # [v, 3, h, w]; [v, h, w] x 2
    r = (r.detach().cpu().numpy() * 255).clip(0, 255).astype(np.uint8)
    strip = np.ascontiguousarray(r.transpose(2, 0, 3, 1).reshape(h, v * w, 3))      # "v c h w -> h (v w) c"
    if return_aux:
        return (strip,) + tuple(np.ascontiguousarray(m.transpose(1, 0, 2).reshape(h, v * w)) for m in maps)
    return strip


def render_generic(pc, c2ws, fxfycxcy, h=512, w=512, backend=None, return_aux=False):
    """gs_core.py:1300-1316: `pc` a GaussianModel, c2ws [v, 4, 4], fxfycxcy [v, 4] -> uint8 [v, h, w, 3].  The reference loops
    render_opencv_cam over the views; here they are one batched launch sequence.
    return_aux=True -> (images, depth float32 [v, h, w], alpha float32 [v, h, w]) from the same render."""
    from .raster import default_backend
    dev = pc._xyz.device
    c = torch.as_tensor(c2ws).float().to(dev)[None]
    k = torch.as_tensor(fxfycxcy).float().to(dev)[None]
    be = backend if backend is not None else default_backend()
    with torch.no_grad():
        r = be.render_views(pc._xyz.float()[None], pc.get_features.float()[None], pc._scaling.float()[None], pc._rotation.float()[None],
                            pc._opacity.float()[None], h, w, c, k, **(dict(aux=True) if return_aux else {}))
    r, maps = (r[0][0], [m[0, :, 0].detach().cpu().numpy() for m in r[1:]]) if return_aux else (r[0], None)   # [v, 3, h, w]; [v, h, w] x 2
    r = (r.detach().cpu().numpy() * 255).clip(0, 255).astype(np.uint8)
    img = np.ascontiguousarray(r.transpose(0, 2, 3, 1))                                    # "v c h w -> v h w c"
    return (img,) + tuple(maps) if return_aux else img


def construct_dtypes(pc, enable_gs_viewer=True):
    """gs_core.py:578-606 (fp32 variant; PLY has no 16-bit float type)."""
    l = [("x", "f4"), ("y", "f4"), ("z", "f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")]
    l += [(f"f_dc_{i}", "f4") for i in range(pc._features_dc.shape[1] * pc._features_dc.shape[2])]
    if enable_gs_viewer:
        assert pc.sh_degree <= 3, "GS viewer only supports SH up to degree 3"
        l += [(f"f_rest_{i}", "f4") for i in range(((3 + 1) ** 2 - 1) * 3)]
    elif pc.sh_degree > 0:
        l += [(f"f_rest_{i}", "f4") for i in range(pc._features_rest.shape[1] * pc._features_rest.shape[2])]
    l.append(("opacity", "f4"))
    l += [(f"scale_{i}", "f4") for i in range(pc._scaling.shape[1])]
    l += [(f"rot_{i}", "f4") for i in range(pc._rotation.shape[1])]
    return l


def save_ply(pc, path, enable_gs_viewer=True, filter_mask=None):
    """gs_core.py:636-712: raw (pre-activation) parameters, DC colour also as 8-bit rgb, f_rest zero-padded to SH degree 3."""
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    n = lambda t: t.detach().float().cpu().numpy()
    xyz = n(pc._xyz)
    f_dc = n(pc._features_dc.transpose(1, 2).flatten(start_dim=1))
    rgb = ((f_dc * C0 + 0.5) * 255.0).clip(0.0, 255.0).astype(np.uint8)
    if pc.scaling_modifier is not None:
        scale = np.log(n(pc.get_scaling))
    else:
        scale = n(pc._scaling)
    f_rest = n(pc._features_rest.transpose(1, 2).flatten(start_dim=1)) if pc.sh_degree > 0 else None
    if enable_gs_viewer:
        full = np.zeros((xyz.shape[0], 3 * ((3 + 1) ** 2 - 1)), dtype=np.float32)
        if f_rest is not None:
            full[:, :f_rest.shape[1]] = f_rest
        f_rest = full
    dtype = construct_dtypes(pc, enable_gs_viewer)
    el = np.empty(xyz.shape[0], dtype=dtype)
    cols = [xyz, rgb, f_dc] + ([f_rest] if f_rest is not None else []) + [n(pc._opacity), scale, n(pc._rotation)]
    names = [name for name, _ in dtype]
    i = 0
    for block in cols:
        for c in range(block.shape[1]):
            el[names[i]] = block[:, c]
            i += 1
    assert i == len(names)
    if filter_mask is not None:
        el = el[np.asarray(filter_mask)]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {el.shape[0]}"]
    header += [f"property {_PLY_TYPES[t]} {name}" for name, t in dtype] + ["end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(el.astype(el.dtype.newbyteorder("<"), copy=False).tobytes())


def read_ply(path):
    """-> structured array of the 'vertex' element (binary little endian, scalar float / uchar properties)."""
    rev = {"float": "<f4", "float32": "<f4", "uchar": "u1", "uint8": "u1", "double": "<f8", "float64": "<f8", "int": "<i4", "int32": "<i4"}
    with open(path, "rb") as f:
        assert f.readline().strip() == b"ply"
        fmt = f.readline().split()
        assert fmt[:2] == [b"format", b"binary_little_endian"], "only binary little-endian files (what save_ply writes)"
        count, props, in_vertex = 0, [], False
        for line in iter(f.readline, b""):
            tok = line.decode("ascii").split()
            if tok[0] == "end_header":
                break
            if tok[0] == "element":
                in_vertex = tok[1] == "vertex"
                if in_vertex:
                    count = int(tok[2])
            elif tok[0] == "property" and in_vertex:
                props.append((tok[2], rev[tok[1]]))
        return np.frombuffer(f.read(count * np.dtype(props).itemsize), dtype=props, count=count)


def load_ply(pc, path, device="cpu"):
    """gs_core.py:715-760: fills `pc` (raw parameters) from a file written by save_ply / any 3DGS exporter."""
    v = read_ply(path)
    xyz = np.stack((v["x"], v["y"], v["z"]), axis=1)
    dc = np.stack((v["f_dc_0"], v["f_dc_1"], v["f_dc_2"]), axis=1)[:, :, None]                      # [P, 3, 1]
    idx = lambda prefix: sorted((n for n in v.dtype.names if n.startswith(prefix)), key=lambda s: int(s.split("_")[-1]))
    feats = dc
    if pc.sh_degree > 0:
        k = 3 * (pc.sh_degree + 1) ** 2 - 3
        extra = np.stack([v[n] for n in idx("f_rest_")[:k]], axis=1).reshape(xyz.shape[0], 3, (pc.sh_degree + 1) ** 2 - 1)
        feats = np.concatenate((dc, extra), axis=2)
    scales = np.stack([v[n] for n in idx("scale_")], axis=1)
    rots = np.stack([v[n] for n in idx("rot_")], axis=1)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=device)
    return pc.set_data(t(xyz), t(feats).transpose(1, 2).contiguous(), t(scales), t(rots), t(v["opacity"][:, None]))


def field_tables(resolution, num_blocks, relax_ratio=1.5):
    """The grid of gs_core.py:809-824, on the host in fp32 with the reference's own expressions: lin [R] = linspace(-1, 1, R), and per
    block index the exclusive bounds lo / hi [nb] of a member's coordinate (the chunk's first / last coordinate -/+ block_size *
    relax_ratio).  A tensor minus a Python scalar is one fp32 operation on the rounded scalar, as `vmin -= ...` is."""
    block_size = 2 / num_blocks
    lin = torch.linspace(-1, 1, resolution)
    chunks = lin.split(resolution // num_blocks)
    lo = torch.stack([c.min() for c in chunks]) - block_size * relax_ratio
    hi = torch.stack([c.max() for c in chunks]) + block_size * relax_ratio
    return lin, lo, hi


def extract_fields(pc, resolution=128, num_blocks=16, relax_ratio=1.5, lib=None):
    """gs_core.py:786-852: `pc` a GaussianModel -> occ [R, R, R] float32 on its device, indexed [x, y, z]; sets pc.mesh_center
    (tensor [3]) and pc.mesh_scale (float) as the reference does.  One call of dgs_gaussian_field (include/dgs_field.h) on the
    current stream; membership in a block is decided by comparing the fp32 numbers formed here with the reference's expressions."""
    from . import _native
    block_size = 2 / num_blocks
    assert resolution % block_size == 0
    if resolution % num_blocks != 0:
        raise ValueError(f"extract_fields: resolution {resolution} is not a multiple of num_blocks {num_blocks}")
    with torch.no_grad():
        xyz = pc.get_xyz.float()
        if xyz.shape[0] == 0:
            raise ValueError("extract_fields: no Gaussians (all filtered away?)")
        mn, mx = xyz.amin(0), xyz.amax(0)
        pc.mesh_center = (mn + mx) / 2
        pc.mesh_scale = 1.8 / (mx - mn).amax().item()
        dev = xyz.device
        xyzs = ((xyz - pc.mesh_center) * pc.mesh_scale).contiguous()
        lin, lo, hi = (t.to(dev).contiguous() for t in field_tables(resolution, num_blocks, relax_ratio))
        scaling, rotation, opacity = (t.detach().float().contiguous() for t in (pc._scaling, pc._rotation, pc._opacity))
        occ = torch.empty([resolution] * 3, dtype=torch.float32, device=dev)
        L = lib or _native.lib()
        a = _native.DgsFieldArgs()
        a.N, a.R, a.nb, a.split = xyz.shape[0], resolution, num_blocks, resolution // num_blocks
        a.mesh_scale = pc.mesh_scale
        a.scaling_modifier = 1.0 if pc.scaling_modifier is None else float(pc.scaling_modifier)
        a.workspace_bytes = L.dgs_gaussian_field_workspace_bytes(a.N, a.nb)
        if a.workspace_bytes <= 0:
            raise ValueError(f"extract_fields: unsupported grid (num_blocks {num_blocks})")
        ws = torch.empty(a.workspace_bytes, dtype=torch.uint8, device=dev)
        a.xyz, a.scaling, a.rotation, a.opacity, a.lin, a.lo, a.hi, a.occ, a.workspace = (
            ctypes.c_void_p(t.data_ptr()) for t in (xyzs, scaling, rotation, opacity, lin, lo, hi, occ, ws))
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if xyz.is_cuda else None
        rc = L.dgs_gaussian_field(ctypes.byref(a), stream)
        if rc != 0:
            raise ValueError(f"dgs_gaussian_field failed: {rc} ({_native.status_string(L, rc)})") if rc == -1 else RuntimeError(
                f"dgs_gaussian_field failed: {rc} ({_native.status_string(L, rc)})")
        if xyz.is_cuda:
            for t in (xyzs, scaling, rotation, opacity, lin, lo, hi, ws):
                t.record_stream(torch.cuda.current_stream(dev))
    return occ


class Mesh:
    """What GaussianModel.extract_mesh returns: vertices float32 [V, 3] in the reference's normalised cube [-1, 1]^3 and faces int32
    [F, 3], both on the model's device (the reference wraps the same two arrays in a trimesh.Trimesh)."""

    def __init__(self, vertices, faces, colors=None, normals=None, density=None):
        self.vertices, self.faces = vertices, faces
        self.colors, self.normals, self.density = colors, normals, density      # per vertex, of extract_mesh(attributes=True); else None

    def __repr__(self):
        return f"Mesh(vertices={tuple(self.vertices.shape)}, faces={tuple(self.faces.shape)}, device={self.vertices.device})"


def _check_rc(L, rc, name):
    """The return code of a C call: -1 (an invalid argument) is a ValueError, every other failure a RuntimeError."""
    if rc != 0:
        from . import _native
        raise (ValueError if rc == -1 else RuntimeError)(f"{name} failed: {rc} ({_native.status_string(L, rc)})")


def _check_mesh(who, vertices, faces):
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32:
        raise ValueError(f"{who}: vertices must be float32 [V, 3], got {vertices.dtype} {tuple(vertices.shape)}")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError(f"{who}: faces must be int32 [F, 3], got {faces.dtype} {tuple(faces.shape)}")
    if faces.device != vertices.device:
        raise ValueError(f"{who}: vertices on {vertices.device}, faces on {faces.device}")


class _MeshCall:
    """What the C calls of one mesh stage need: the checked, detached, contiguous mesh, the library, a workspace, the current stream and
    the stage's argument block `a` with V, F, vertices, faces, workspace and workspace_bytes filled in.  `symbols` and `feature` are
    for a library that predates the stage, `args` is the type of the block, `size(L, a)` the workspace size and `limit` says what
    sizes the stage takes.  A caller with parameters of its own calls _check_mesh first, so that the mesh is complained about first."""

    def __init__(self, who, vertices, faces, lib, symbols, feature, args, size, limit):
        from . import _native
        _check_mesh(who, vertices, faces)
        self.who, self._native = who, _native
        self.L = L = lib or _native.lib()
        if not all(hasattr(L, name) for name in symbols):
            raise RuntimeError(f"{who}: this build of the library predates {feature} -- rebuild it (`python -m dgs_amd.build`)")
        self.vertices, self.faces = vertices.detach().contiguous(), faces.detach().contiguous()
        self.dev = vertices.device
        self.a = a = args()
        a.V, a.F = self.vertices.shape[0], self.faces.shape[0]
        a.workspace_bytes = size(L, a)
        if a.workspace_bytes <= 0:
            raise ValueError(f"{who}: unsupported size V = {a.V}, F = {a.F} ({limit})")
        self.ws = torch.empty(a.workspace_bytes, dtype=torch.uint8, device=self.dev)
        a.workspace = ctypes.c_void_p(self.ws.data_ptr())
        a.vertices = ctypes.c_void_p(self.vertices.data_ptr()) if a.V else None
        a.faces = ctypes.c_void_p(self.faces.data_ptr()) if a.F else None
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream) if vertices.is_cuda else None

    def call(self, name):
        _check_rc(self.L, getattr(self.L, name)(ctypes.byref(self.a), self.stream), name)

    def done(self, *more):
        """After the last call: the mesh, the workspace and `more` (a None among them is skipped) are in use on the current stream."""
        if self.vertices.is_cuda:
            for t in (self.vertices, self.faces, self.ws) + more:
                if t is not None:
                    t.record_stream(torch.cuda.current_stream(self.dev))


def marching_cubes(occ, level, lib=None):
    """The counterpart of `mcubes.marching_cubes(occ, level)` on occ's device: occ float32 [X, Y, Z] -> (vertices float32 [V, 3] in
    index coordinates, triangles int32 [F, 3]), in the canonical order of include/dgs_mesh.h (csrc/mesh.hip); a sample is inside iff
    occ > level.  dgs_marching_cubes_count, ONE readback of {V, F} to size the outputs, dgs_marching_cubes_emit; no crossing gives two
    empty tensors."""
    from . import _native
    if occ.dim() != 3 or occ.dtype != torch.float32:
        raise ValueError(f"marching_cubes: occ must be float32 [X, Y, Z], got {occ.dtype} {tuple(occ.shape)}")
    with torch.no_grad():
        occ = occ.detach().contiguous()
        dev = occ.device
        L = lib or _native.lib()
        a = _native.DgsMeshArgs()
        a.X, a.Y, a.Z = occ.shape
        a.level = float(level)
        a.workspace_bytes = L.dgs_marching_cubes_workspace_bytes(a.X, a.Y, a.Z)
        if a.workspace_bytes <= 0:
            raise ValueError(f"marching_cubes: unsupported grid {tuple(occ.shape)} (every axis >= 2, at most 2^30 samples)")
        ws = torch.empty(a.workspace_bytes, dtype=torch.uint8, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)              # the call writes uint32 [2]
        a.occ, a.counts, a.workspace = (ctypes.c_void_p(t.data_ptr()) for t in (occ, counts, ws))
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if occ.is_cuda else None
        _check_rc(L, L.dgs_marching_cubes_count(ctypes.byref(a), stream), "dgs_marching_cubes_count")
        nv, nf = (c & 0xFFFFFFFF for c in counts.tolist())                  # the feature's one host synchronisation
        vertices = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        triangles = torch.empty((nf, 3), dtype=torch.int32, device=dev)
        if nv:
            a.vertices, a.triangles = ctypes.c_void_p(vertices.data_ptr()), ctypes.c_void_p(triangles.data_ptr())
            a.max_vertices, a.max_triangles = nv, nf
            _check_rc(L, L.dgs_marching_cubes_emit(ctypes.byref(a), stream), "dgs_marching_cubes_emit")
        if occ.is_cuda:
            for t in (occ, ws, counts):
                t.record_stream(torch.cuda.current_stream(dev))
    return vertices, triangles


def remove_small_components(vertices, faces, min_f=64, min_d=20, return_labels=False, lib=None):
    """The two floater filters of the reference's clean_mesh on the mesh's device (include/dgs_mesh_clean.h, csrc/mesh_clean.hip):
    a connected component (faces sharing vertex indices) goes when it has fewer than min_f faces (0 = off) or when the diagonal of its
    bounding box is below min_d percent of the mesh's (0 = off); vertices no kept face refers to go with it.  The defaults are the
    reference's values.  vertices float32 [V, 3], faces int32 [F, 3] -> (vertices', faces') in input order, faces renumbered; with
    return_labels also labels int32 [F], the smallest vertex index of each input face's component (-1: an index outside [0, V)).
    dgs_mesh_clean_count, ONE readback of the five counts to size the outputs, dgs_mesh_clean_emit."""
    from . import _native
    _check_mesh("remove_small_components", vertices, faces)
    if int(min_f) != min_f or min_f < 0 or not min_d >= 0:
        raise ValueError(f"remove_small_components: min_f must be an integer >= 0 and min_d a percentage >= 0, got {min_f}, {min_d}")
    with torch.no_grad():
        m = _MeshCall("remove_small_components", vertices, faces, lib, _native.MESH_CLEAN_SYMBOLS, "the mesh clean-up", _native.DgsMeshCleanArgs,
                      lambda L, a: L.dgs_mesh_clean_workspace_bytes(a.V, a.F), "at most 2^30 each")
        a, dev = m.a, m.dev
        a.min_faces, a.min_diag_pct = int(min_f), float(min_d)
        counts = torch.empty(5, dtype=torch.int32, device=dev)              # the call writes uint32 [5]
        a.counts = ctypes.c_void_p(counts.data_ptr())
        m.call("dgs_mesh_clean_count")
        nv, nf = (c & 0xFFFFFFFF for c in counts.tolist()[:2])              # the feature's one host synchronisation
        out_v = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        out_f = torch.empty((nf, 3), dtype=torch.int32, device=dev)
        labels = torch.empty(a.F, dtype=torch.int32, device=dev) if return_labels else None
        if nf or (return_labels and a.F):
            a.out_vertices = ctypes.c_void_p(out_v.data_ptr()) if nv else None
            a.out_faces = ctypes.c_void_p(out_f.data_ptr()) if nf else None
            a.labels = ctypes.c_void_p(labels.data_ptr()) if return_labels else None
            a.max_vertices, a.max_faces = nv, nf
            m.call("dgs_mesh_clean_emit")
        m.done(counts)
    return (out_v, out_f, labels) if return_labels else (out_v, out_f)


class _Clustering(_MeshCall):
    """The mesh, the library and one workspace large enough for every n up to n_max: count(n) as often as the caller likes (one
    readback of the five counts each), then emit() at the n counted last."""

    def __init__(self, vertices, faces, n_max, lib, who):
        from . import _native
        _check_mesh(who, vertices, faces)
        if int(n_max) != n_max or not 1 <= n_max <= 1024:
            raise ValueError(f"{who}: the grid must have an integer number of cells per axis in [1, 1024], got {n_max}")
        super().__init__(who, vertices, faces, lib, _native.MESH_DECIMATE_SYMBOLS, "the mesh decimation", _native.DgsMeshDecimateArgs,
                         lambda L, a: L.dgs_mesh_decimate_workspace_bytes(a.V, a.F, int(n_max)),    # grows with n: enough for every n <= n_max
                         "at most 2^30 each")
        self.counts_dev = torch.empty(5, dtype=torch.int32, device=self.dev)  # the call writes uint32 [5]
        self.a.counts = ctypes.c_void_p(self.counts_dev.data_ptr())
        self.counts = None

    def count(self, n):
        """-> [V', F', degenerate, duplicates dropped, invalid] at n cells per axis; a host synchronisation."""
        self.a.n = int(n)
        self.call("dgs_mesh_decimate_count")
        self.counts = [c & 0xFFFFFFFF for c in self.counts_dev.tolist()]
        if self.counts[0] == 0xFFFFFFFF:
            raise RuntimeError(f"{self.who}: dgs_mesh_decimate_count found no slot for a face in its table")
        return self.counts

    def emit(self):
        nv, nf = self.counts[:2]
        out_v = torch.empty((nv, 3), dtype=torch.float32, device=self.dev)
        out_f = torch.empty((nf, 3), dtype=torch.int32, device=self.dev)
        if nf:
            a = self.a
            a.out_vertices, a.out_faces = ctypes.c_void_p(out_v.data_ptr()), ctypes.c_void_p(out_f.data_ptr())
            a.max_vertices, a.max_faces = nv, nf
            self.call("dgs_mesh_decimate_emit")
        self.done(self.counts_dev)
        return out_v, out_f


def cluster_vertices(vertices, faces, n, return_counts=False, lib=None):
    """Vertex clustering on a uniform grid of n cells along the longest axis of the mesh's box, on the mesh's device
    (include/dgs_mesh_decimate.h, csrc/mesh_decimate.hip; MeshLab's meshing_decimation_clustering with the null and duplicate faces
    removed): the vertices of one cell become one vertex at their mean, faces with two corners in one cell go, of faces with the same
    three cells the one of the smallest index stays; clusters no kept face refers to are not output.  vertices float32 [V, 3], faces
    int32 [F, 3] -> (vertices' in ascending cell order, faces' in input order with their orientation); with return_counts also
    [V', F', degenerate faces, duplicate faces dropped, invalid faces].  The same input gives the same bytes.  Clustering can leave
    non-manifold edges where a thin part collapses.  dgs_mesh_decimate_count, ONE readback of the five counts,
    dgs_mesh_decimate_emit."""
    with torch.no_grad():
        c = _Clustering(vertices, faces, n, lib, "cluster_vertices")
        counts = c.count(n)
        out_v, out_f = c.emit()
    return (out_v, out_f, counts) if return_counts else (out_v, out_f)


def decimate_mesh(vertices, faces, target, n_max=1024, return_n=False, lib=None):
    """The counterpart of the reference's decimate_mesh(verts, faces, target) (mesh_utils.py:44-85) on the mesh's device, by vertex
    clustering (cluster_vertices) instead of pymeshlab's quadric edge collapse.  If target <= 0 or F <= target the inputs come back
    unchanged (the reference's own condition).  Otherwise the result has AT MOST `target` faces, at the grid size n this bisection
    finds and nothing else: lo = 1, hi = n_max + 1; while hi - lo > 1: mid = (lo + hi) // 2, lo = mid if F'(mid) <= target else
    hi = mid; n = lo.  F'(1) = 0, so F'(lo) <= target holds throughout.  F'(n) is not monotone in n, so n is not promised to be the
    largest grid that meets the target.  At most 10 counts (dgs_mesh_decimate_count) with a readback of five integers each, then one
    emit; the mesh never leaves the device.  With return_n also n (0 when the inputs came back)."""
    if not target >= 0 and not target < 0:
        raise ValueError(f"decimate_mesh: target must be a number, got {target}")
    if target <= 0 or faces.shape[0] <= target:
        return (vertices, faces, 0) if return_n else (vertices, faces)
    with torch.no_grad():
        c = _Clustering(vertices, faces, n_max, lib, "decimate_mesh")
        lo, hi, last = 1, int(n_max) + 1, None
        while hi - lo > 1:
            mid = last = (lo + hi) // 2
            if c.count(mid)[1] <= target:
                lo = mid
            else:
                hi = mid
        if last != lo:                                                     # the workspace holds another n's count
            c.count(lo)
        out_v, out_f = c.emit()
    return (out_v, out_f, lo) if return_n else (out_v, out_f)


def smooth_mesh(vertices, faces, iterations=10, lam=0.5, mu=-0.53, fixed=None, return_counts=False, lib=None):
    """Taubin smoothing of the vertices on the mesh's device (include/dgs_mesh_smooth.h, csrc/mesh_smooth.hip; MeshLab's
    apply_coord_taubin_smoothing with the cotangent weights off, the commented alternative of the remeshing in the reference's
    clean_mesh / decimate_mesh, at MeshLab's defaults): `iterations` times a pass with weight lam, then one with weight mu, each moving
    every vertex towards (lam > 0) or away from (mu < 0) the mean of the other corners of its faces, all reads from the pass's input.
    mu = 0 is plain Laplacian smoothing, which shrinks the object.  vertices float32 [V, 3], faces int32 [F, 3], fixed None or a
    bool / uint8 [V] of vertices that stay -> vertices float32 [V, 3] on the same device; the faces are untouched.  Invalid faces (an
    index outside [0, V)) and null faces (two equal indices) are ignored; a vertex no such face names, or one that more than 16,384
    name, keeps its bytes.  With return_counts also [invalid faces, null faces, vertices over that cap, unreferenced vertices], the
    call's only host synchronisation.  The same input gives the same bytes.  Not part of this: border handling (an open mesh shrinks
    at its border), cotangent weights, remeshing, non-manifold repair (repair_mesh, before this).  One C call on the current stream."""
    from . import _native
    _check_mesh("smooth_mesh", vertices, faces)
    if int(iterations) != iterations or not 0 <= iterations <= 1 << 20:
        raise ValueError(f"smooth_mesh: iterations must be an integer in [0, 2^20], got {iterations}")
    if not (math.isfinite(lam) and math.isfinite(mu)):
        raise ValueError(f"smooth_mesh: lam and mu must be finite, got {lam}, {mu}")
    if fixed is not None:
        if fixed.dim() != 1 or fixed.shape[0] != vertices.shape[0] or fixed.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"smooth_mesh: fixed must be bool or uint8 [V] = [{vertices.shape[0]}], got {fixed.dtype} {tuple(fixed.shape)}")
        if fixed.device != vertices.device:
            raise ValueError(f"smooth_mesh: vertices on {vertices.device}, fixed on {fixed.device}")
    with torch.no_grad():
        m = _MeshCall("smooth_mesh", vertices, faces, lib, _native.MESH_SMOOTH_SYMBOLS, "the mesh smoothing", _native.DgsMeshSmoothArgs,
                      lambda L, a: L.dgs_mesh_smooth_workspace_bytes(a.V, a.F), "at most 2^30 and 2^29")
        a = m.a
        if fixed is not None:
            fixed = fixed.detach().contiguous().view(torch.uint8)           # a bool is one byte, 0 or 1
        a.lam, a.mu, a.iterations = float(lam), float(mu), int(iterations)
        out = torch.empty((a.V, 3), dtype=torch.float32, device=m.dev)
        counts = torch.empty(4, dtype=torch.int32, device=m.dev) if return_counts else None   # the call writes uint32 [4]
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
        a.fixed, a.out_vertices, a.counts = ptr(fixed), ptr(out), ptr(counts)
        m.call("dgs_mesh_smooth")
        m.done(fixed)
        if return_counts:
            return out, [c & 0xFFFFFFFF for c in counts.tolist()]           # the one host synchronisation
    return out


def _repair_call(vertices, faces, lib, who):
    """The _MeshCall of dgs_mesh_repair_count / _emit / dgs_mesh_topology."""
    from . import _native
    return _MeshCall(who, vertices, faces, lib, _native.MESH_REPAIR_SYMBOLS, "the mesh repair", _native.DgsMeshRepairArgs,
                     lambda L, a: L.dgs_mesh_repair_workspace_bytes(a.V, a.F), "at most 2^30 and 2^28")


def repair_mesh(vertices, faces, return_counts=False, lib=None):
    """The four repair filters of the reference's clean_mesh (repair=True) on the mesh's device (include/dgs_mesh_repair.h,
    csrc/mesh_repair.hip; MeshLab's meshing_remove_null_faces, meshing_remove_duplicate_faces, meshing_repair_non_manifold_edges with
    method 0 and meshing_repair_non_manifold_vertices with vertdispratio 0, in their order-free form): faces with an index outside
    [0, V), with two equal indices or without area go; of the faces on the same three vertices the one of the smallest index stays; on
    an edge of three or more faces the two largest stay (ties: the smaller index) and the others go; a vertex whose faces form several
    fans keeps the fan of its first corner and gets one copy, the same 12 bytes, for each other fan; vertices no face names go.
    vertices float32 [V, 3], faces int32 [F, 3] -> (vertices', faces') on the same device: the kept vertices in input order, then the
    copies; the kept faces in input order, with their orientation.  A manifold mesh without such faces and vertices comes back byte for
    byte.  With return_counts also a dict of the ten counts (_native.MESH_REPAIR_COUNTS: vertices, faces, invalid_faces, null_faces,
    duplicate_faces, non_manifold_edges, faces_removed, non_manifold_vertices, vertices_added, unreferenced_vertices).  The same input
    gives the same bytes.  Orientation is neither checked nor repaired; an edge that kept a face which another edge removed becomes a
    border.  dgs_mesh_repair_count, ONE readback of the ten counts to size the outputs, dgs_mesh_repair_emit."""
    with torch.no_grad():
        r = _repair_call(vertices, faces, lib, "repair_mesh")
        counts_dev = torch.empty(len(r._native.MESH_REPAIR_COUNTS), dtype=torch.int32, device=r.dev)   # the call writes uint32 [10]
        r.a.counts = ctypes.c_void_p(counts_dev.data_ptr())
        r.call("dgs_mesh_repair_count")
        counts = [c & 0xFFFFFFFF for c in counts_dev.tolist()]              # the feature's one host synchronisation
        if counts[0] == 0xFFFFFFFF:
            raise RuntimeError("repair_mesh: dgs_mesh_repair_count found no slot for a face or an edge in its tables")
        nv, nf = counts[:2]
        out_v = torch.empty((nv, 3), dtype=torch.float32, device=r.dev)
        out_f = torch.empty((nf, 3), dtype=torch.int32, device=r.dev)
        if nf:
            r.a.out_vertices, r.a.out_faces = ctypes.c_void_p(out_v.data_ptr()), ctypes.c_void_p(out_f.data_ptr())
            r.a.max_vertices, r.a.max_faces = nv, nf
            r.call("dgs_mesh_repair_emit")
        r.done(counts_dev)
    return (out_v, out_f, dict(zip(r._native.MESH_REPAIR_COUNTS, counts))) if return_counts else (out_v, out_f)


def mesh_topology(vertices, faces, lib=None):
    """The census of include/dgs_mesh_repair.h (dgs_mesh_topology) on the mesh's device -> a dict of integers
    (_native.MESH_TOPOLOGY_COUNTS): border_edges (one face), manifold_edges (two), non_manifold_edges (three or more),
    non_manifold_vertices (the faces around the vertex, joined through its edges of exactly two faces, form more than one fan),
    referenced_vertices, faces, euler_characteristic (referenced vertices - edges + faces), over the faces whose three indices lie in
    [0, V) and differ; a face that occurs twice counts twice, and the coordinates are not read.  It decides nothing for repair_mesh:
    it is the check of a raw mesh (is a repair needed?) as well as of a repaired one.  One C call and one readback of seven integers."""
    with torch.no_grad():
        r = _repair_call(vertices, faces, lib, "mesh_topology")
        out = torch.empty(len(r._native.MESH_TOPOLOGY_COUNTS), dtype=torch.int64, device=r.dev)
        r.a.topology = ctypes.c_void_p(out.data_ptr())
        r.call("dgs_mesh_topology")
        numbers = out.tolist()                                              # the host synchronisation
        r.done(out)
        if numbers[0] < 0:
            raise RuntimeError("mesh_topology: dgs_mesh_topology found no slot for an edge in its table")
    return dict(zip(r._native.MESH_TOPOLOGY_COUNTS, numbers))


def mesh_attributes(pc, points, num_blocks=64, reach=2, attr=None, want=("colors", "normals", "density"), lib=None):
    """What the Gaussians of `pc` say at `points` float32 [V, 3] of the normalised cube [-1, 1]^3 (the vertices of extract_mesh): a dict
    with the entries of `want`, on pc's device --
        "density"  [V]     sum of sigmoid(opacity) * exp(power) over the Gaussians in the window of `reach` cells (pitch 2 / num_blocks)
                           around the point's cell,
        "colors"   [V, 3]  the mean of `attr` [N, 3] under those weights, 0 where the density is 0; attr defaults to the
                           view-independent colour clamp(0.5 + C0 * f_dc, 0, 1), the reference's SH2RGB at degree 0,
        "normals"  [V, 3]  -gradient / |gradient| of the density, 0 where the gradient is 0: it points out of the object, to the side
                           the faces of marching_cubes turn to.
    The definition and the summation order are in include/dgs_mesh_attr.h (csrc/mesh_attr.hip): the same inputs give the same bytes,
    and a point's values do not depend on the other points of the call.  The centres are normalised with the expressions of
    extract_fields, and pc.mesh_center / pc.mesh_scale are set the same way, so the call stands on its own.  One C call on the current
    stream, no host synchronisation."""
    from . import _native
    want = tuple(want)
    if not want or any(w not in ("colors", "normals", "density") for w in want):
        raise ValueError(f"mesh_attributes: want must name some of 'colors', 'normals', 'density', got {want}")
    if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise ValueError(f"mesh_attributes: points must be float32 [V, 3], got {points.dtype} {tuple(points.shape)}")
    with torch.no_grad():
        xyz = pc.get_xyz.float()
        if xyz.shape[0] == 0:
            raise ValueError("mesh_attributes: no Gaussians (all filtered away?)")
        if points.device != xyz.device:
            raise ValueError(f"mesh_attributes: the model on {xyz.device}, points on {points.device}")
        L = lib or _native.lib()
        if not all(hasattr(L, name) for name in _native.MESH_ATTR_SYMBOLS):
            raise RuntimeError("mesh_attributes: this build of the library predates the mesh attributes -- rebuild it (`python -m dgs_amd.build`)")
        mn, mx = xyz.amin(0), xyz.amax(0)
        pc.mesh_center = (mn + mx) / 2
        pc.mesh_scale = 1.8 / (mx - mn).amax().item()
        dev = xyz.device
        xyzs = ((xyz - pc.mesh_center) * pc.mesh_scale).contiguous()
        scaling, rotation, opacity = (t.detach().float().contiguous() for t in (pc._scaling, pc._rotation, pc._opacity))
        if attr is None:
            attr = (0.5 + C0 * pc._features_dc.detach().float().reshape(-1, 3)).clamp(0, 1)
        attr = attr.detach().float().contiguous()
        if attr.shape != (xyz.shape[0], 3) or attr.device != dev:
            raise ValueError(f"mesh_attributes: attr must be [N, 3] = [{xyz.shape[0]}, 3] on {dev}, got {tuple(attr.shape)} on {attr.device}")
        points = points.detach().contiguous()
        a = _native.DgsMeshAttrArgs()
        a.V, a.N, a.nb, a.reach = points.shape[0], xyz.shape[0], int(num_blocks), int(reach)
        a.mesh_scale = pc.mesh_scale
        a.scaling_modifier = 1.0 if pc.scaling_modifier is None else float(pc.scaling_modifier)
        a.workspace_bytes = L.dgs_mesh_attributes_workspace_bytes(a.N, a.nb, a.V)
        if a.workspace_bytes <= 0:
            raise ValueError(f"mesh_attributes: unsupported size (num_blocks {num_blocks} in [1, 256], V = {a.V} at most 2^30)")
        ws = torch.empty(a.workspace_bytes if a.V else 0, dtype=torch.uint8, device=dev)
        density = torch.empty(a.V, dtype=torch.float32, device=dev) if "density" in want else None
        colors = torch.empty((a.V, 3), dtype=torch.float32, device=dev) if "colors" in want else None
        gradient = torch.empty((a.V, 3), dtype=torch.float32, device=dev) if "normals" in want else None
        ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
        a.xyz, a.scaling, a.rotation, a.opacity, a.attr, a.points, a.workspace = (ptr(t) for t in (xyzs, scaling, rotation, opacity, attr, points, ws))
        a.density, a.attr_out, a.gradient = ptr(density), ptr(colors), ptr(gradient)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if xyz.is_cuda else None
        _check_rc(L, L.dgs_mesh_attributes(ctypes.byref(a), stream), "dgs_mesh_attributes")
        if xyz.is_cuda:
            for t in (xyzs, scaling, rotation, opacity, attr, points, ws):
                t.record_stream(torch.cuda.current_stream(dev))
        out = {}
        if colors is not None:
            out["colors"] = colors
        if gradient is not None:
            norm = torch.sqrt((gradient * gradient).sum(dim=1, keepdim=True))
            out["normals"] = torch.where(norm > 0, -gradient / norm, torch.zeros_like(gradient))
        if density is not None:
            out["density"] = density
    return out


def extract_mesh(pc, density_thresh=0.005, resolution=256, num_blocks=64, lib=None, min_f=0, min_d=0, decimate_target=0, attributes=False,
                 smooth_iterations=0, smooth_lambda=0.5, smooth_mu=-0.53, repair=False):
    """gs_core.py:855-869: extract_fields (sets pc.mesh_center / pc.mesh_scale), marching cubes at density_thresh,
    vertices / (resolution - 1) * 2 - 1 -> Mesh on pc's device.  min_f / min_d > 0 then drop the floaters as the first two
    filters of the reference's clean_mesh do (remove_small_components on the mesh in [-1, 1]^3, which is what clean_mesh sees; the
    reference's values are min_f=64, min_d=20); with both 0, the default, that path is not entered.  decimate_target > 0 then brings
    a mesh of more faces down to at most that many by vertex clustering on the device (decimate_mesh; the reference's value is 1e5,
    by pymeshlab's quadric edge collapse); 0, the default, does not enter that path, and with all three 0 the raw level set is
    returned.  repair=True then runs the repair filters of clean_mesh on that mesh (repair_mesh: null and duplicate faces,
    non-manifold edges and vertices, unreferenced vertices; the reference's clean_mesh has repair=True as its default), so that the
    smoothing and the attributes see the repaired mesh; False, the default, does not enter that path.  The rest of clean_mesh
    (merging close vertices, remeshing: pymeshlab) is not part of this: hand it
    mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy().  smooth_iterations > 0 then smooths the vertices of that
    mesh with that many Taubin iterations of weights smooth_lambda, smooth_mu (smooth_mesh: the commented alternative of the reference's
    remeshing; the faces stay); 0, the default, does not enter that path.  attributes=True then evaluates mesh_attributes at the
    final vertices (same num_blocks, reach 2) and returns them as mesh.colors / mesh.normals / mesh.density; False, the default,
    launches nothing for them and leaves the three None."""
    occ = extract_fields(pc, resolution, num_blocks, lib=lib)
    vertices, triangles = marching_cubes(occ, density_thresh, lib=lib)
    vertices = vertices / (resolution - 1.0) * 2 - 1
    if min_f or min_d:
        vertices, triangles = remove_small_components(vertices, triangles, min_f=min_f, min_d=min_d, lib=lib)
    if decimate_target:
        vertices, triangles = decimate_mesh(vertices, triangles, decimate_target, lib=lib)
    if repair:
        vertices, triangles = repair_mesh(vertices, triangles, lib=lib)
    if smooth_iterations:
        vertices = smooth_mesh(vertices, triangles, smooth_iterations, smooth_lambda, smooth_mu, lib=lib)
    if attributes:
        at = mesh_attributes(pc, vertices, num_blocks=num_blocks, lib=lib)
        return Mesh(vertices, triangles, at["colors"], at["normals"], at["density"])
    return Mesh(vertices, triangles)


def mesh_color_bytes(colors):
    """float colours -> uint8 as the PLY stores them: floor(clamp(c, 0, 1) * 255 + 0.5), evaluated in fp64; a NaN (the colour of a
    vertex at a NaN point) becomes 0."""
    c = np.asarray(colors, dtype=np.float64)
    c = np.clip(np.where(np.isnan(c), 0.0, c), 0.0, 1.0)
    return np.floor(c * 255.0 + 0.5).astype(np.uint8)


def save_mesh_ply(path, vertices, faces, colors=None, normals=None):
    """Binary little-endian PLY: element vertex (x y z float; with `normals` [V, 3] also nx ny nz float; with `colors` [V, 3] also
    red green blue uchar -- float colours go through mesh_color_bytes, uint8 ones are written as they are), element face (list uchar
    int vertex_indices), triangles only.  Without colours and normals the bytes are what this function has always written."""
    n = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    v, f = n(vertices).astype("<f4", copy=False).reshape(-1, 3), n(faces).astype("<i4", copy=False).reshape(-1, 3)
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    el = np.empty(f.shape[0], dtype=[("n", "u1"), ("i", "<i4", (3,))])
    el["n"], el["i"] = 3, f
    fields, props = [("p", "<f4", (3,))], ["property float x", "property float y", "property float z"]
    if normals is not None:
        fields.append(("nrm", "<f4", (3,)))
        props += ["property float nx", "property float ny", "property float nz"]
    if colors is not None:
        fields.append(("rgb", "u1", (3,)))
        props += ["property uchar red", "property uchar green", "property uchar blue"]
    vert = np.empty(v.shape[0], dtype=fields)
    vert["p"] = v
    if normals is not None:
        vert["nrm"] = n(normals).astype("<f4", copy=False).reshape(v.shape[0], 3)
    if colors is not None:
        c = n(colors).reshape(v.shape[0], 3)
        vert["rgb"] = c if c.dtype == np.uint8 else mesh_color_bytes(c)
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}"] + props + [
        f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as out:
        out.write(("\n".join(header) + "\n").encode("ascii"))
        out.write(vert.tobytes())
        out.write(el.tobytes())


def load_mesh_ply(path, return_attributes=False):
    """-> (vertices float32 [V, 3], faces int32 [F, 3]) numpy arrays of a file written by save_mesh_ply (float x y z vertices, optionally
    float nx ny nz and uchar red green blue after them, triangle faces as `list uchar int`).  With return_attributes a third item: a
    dict with "normals" float32 [V, 3] and "colors" uint8 [V, 3] where the file has them."""
    with open(path, "rb") as f:
        assert f.readline().strip() == b"ply"
        assert f.readline().split()[:2] == [b"format", b"binary_little_endian"], "only binary little-endian files (what save_mesh_ply writes)"
        counts, props, cur = {}, {}, None
        for line in iter(f.readline, b""):
            tok = line.decode("ascii").split()
            if tok[0] == "end_header":
                break
            if tok[0] == "element":
                cur = tok[1]
                counts[cur], props[cur] = int(tok[2]), []
            elif tok[0] == "property":
                props[cur].append(tok[1:])
        xyz, nrm, rgb = [["float", k] for k in "xyz"], [["float", k] for k in ("nx", "ny", "nz")], [["uchar", k] for k in ("red", "green", "blue")]
        pv = props["vertex"]
        has_n = pv[3:6] == nrm
        has_c = pv[3 + 3 * has_n:] == rgb
        assert list(counts) == ["vertex", "face"] and pv == xyz + nrm * has_n + rgb * has_c, props
        assert props["face"] == [["list", "uchar", "int", "vertex_indices"]], props
        fields = [("p", "<f4", (3,))] + [("nrm", "<f4", (3,))] * has_n + [("rgb", "u1", (3,))] * has_c
        vert = np.frombuffer(f.read(np.dtype(fields).itemsize * counts["vertex"]), dtype=fields)
        el = np.frombuffer(f.read(13 * counts["face"]), dtype=[("n", "u1"), ("i", "<i4", (3,))])
        assert vert.shape[0] == counts["vertex"] and el.shape[0] == counts["face"] and bool((el["n"] == 3).all())
        v, faces = np.ascontiguousarray(vert["p"]).astype(np.float32).reshape(-1, 3), np.ascontiguousarray(el["i"]).astype(np.int32)
        if not return_attributes:
            return v, faces
        attrs = {}
        if has_n:
            attrs["normals"] = np.ascontiguousarray(vert["nrm"]).astype(np.float32)
        if has_c:
            attrs["colors"] = np.ascontiguousarray(vert["rgb"]).astype(np.uint8)
        return v, faces, attrs
