"""Yardstick of the marching-cubes tests (csrc/mesh.hip, include/dgs_mesh.h): a sequential numpy / fp32 restatement of the header's
definition that uses the table tools/make_mc_table.py produces in memory, the inputs, and checks that do not trust that table.

Restatement: numpy's float32 subtraction, division and addition are the correctly rounded IEEE operations, as are the device's under
STRICT_FP, so vertices are compared bit for bit and triangles element by element.

Table-independent checks (check_mesh):
  V = the number of sample pairs (s, s + e_axis) with different inside flags;
  a vertex has two integer coordinates and one, c, with i <= c <= i + 1 for the owner index i (strictly inside where fp32 can tell:
      t = (level - a) / (b - a) lies in (0, 1) when no sample equals the level; (float)i + t may round to an end);
  the fp64 linear interpolant of occ at the vertex is `level` within 2^-23 * (i + 2) * |b - a|: t carries three fp32 roundings of
      relative 2^-24 each (t <= 1), the sum i + t one of at most 2^-24 * (i + 1), together <= 2^-24 * (i + 4) <= 2^-23 * (i + 2);
  every directed mesh edge occurs once; its reverse occurs once unless both its vertices lie on a boundary face of the grid (the same
      face), those are the `open` edges, everything else without a partner is `bad`; no vertex is unreferenced; no triangle repeats an index.
Reads nothing outside the repository."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@functools.lru_cache(maxsize=None)
def table():
    """-> (count [256], edges [256, 5, 3]) from the generator, in memory."""
    import make_mc_table
    t = make_mc_table.table()
    count = np.array([len(x) for x in t], dtype=np.int64)
    edges = np.zeros((256, 5, 3), dtype=np.int64)
    for c, tris in enumerate(t):
        for i, tri in enumerate(tris):
            edges[c, i] = tri
    return count, edges


def inside_of(occ, level):
    return occ > np.float32(level)


def crossings(occ, level):
    """-> [X, Y, Z, 3] bool: sample s owns a crossed edge along the axis (three array comparisons)."""
    ins = inside_of(occ, level)
    c = np.zeros(occ.shape + (3,), dtype=bool)
    c[:-1, :, :, 0] = ins[:-1] != ins[1:]
    c[:, :-1, :, 1] = ins[:, :-1] != ins[:, 1:]
    c[:, :, :-1, 2] = ins[:, :, :-1] != ins[:, :, 1:]
    return c


def cases(occ, level):
    """-> [X - 1, Y - 1, Z - 1] case numbers."""
    ins = inside_of(occ, level).astype(np.int64)
    X, Y, Z = occ.shape
    case = np.zeros((X - 1, Y - 1, Z - 1), dtype=np.int64)
    for k in range(8):
        dx, dy, dz = k >> 2 & 1, k >> 1 & 1, k & 1
        case |= ins[dx:X - 1 + dx, dy:Y - 1 + dy, dz:Z - 1 + dz] << k
    return case


def restatement(occ, level):
    """include/dgs_mesh.h, sequentially: -> (vertices f32 [V, 3], triangles i32 [F, 3])."""
    occ = np.ascontiguousarray(occ, dtype=np.float32)
    level = np.float32(level)
    X, Y, Z = occ.shape
    cross = crossings(occ, level)
    flat = cross.reshape(-1)                                             # order: owner sample's linear index, then axis
    index = np.cumsum(flat) - 1                                          # vertex index where flat
    x, y, z, axis = (a.reshape(-1)[flat] for a in np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), np.arange(3), indexing="ij"))
    va = occ[x, y, z]
    vb = occ[x + (axis == 0), y + (axis == 1), z + (axis == 2)]
    t = (level - va) / (vb - va)                                         # fp32: two subtractions, one division
    assert t.dtype == np.float32
    vertices = np.stack((x, y, z), axis=1).astype(np.float32)
    rows = np.arange(vertices.shape[0])
    vertices[rows, axis] = vertices[rows, axis] + t                      # one fp32 addition
    count, edges = table()
    case = cases(occ, level).reshape(-1)                                 # order: cell's linear index
    cx, cy, cz = (a.reshape(-1) for a in np.meshgrid(np.arange(X - 1), np.arange(Y - 1), np.arange(Z - 1), indexing="ij"))
    e = edges[case]                                                      # [cells, 5, 3]
    ax, r = e >> 2, e & 3
    hi, lo = r >> 1, r & 1
    dx = np.where(ax == 0, 0, hi)
    dy = np.where(ax == 0, hi, np.where(ax == 1, 0, lo))
    dz = np.where(ax == 2, 0, lo)
    owner = (((cx[:, None, None] + dx) * Y + (cy[:, None, None] + dy)) * Z + (cz[:, None, None] + dz)) * 3 + ax
    valid = np.arange(5)[None, :] < count[case][:, None]                 # [cells, 5]: then in the table's order
    tri = index[owner][valid]
    assert bool(flat[owner][valid].all())                                # the table only names crossed edges
    return vertices, tri.astype(np.int32)


def signed_volume(vertices, triangles):
    v = vertices.astype(np.float64)
    a, b, c = v[triangles[:, 0]], v[triangles[:, 1]], v[triangles[:, 2]]
    return float((a * np.cross(b, c)).sum() / 6.0)


def edge_balance(vertices, triangles, shape):
    """-> (edges (undirected, of closed pairs and open ones), open, bad, repeated directed edges)."""
    V = max(int(vertices.shape[0]), 1)
    t = triangles.astype(np.int64)
    d = np.concatenate((t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]))
    key = d[:, 0] * V + d[:, 1]
    uniq, n = np.unique(key, return_counts=True)
    repeated = int((n > 1).sum())
    rev = d[:, 1] * V + d[:, 0]
    lonely = ~np.isin(rev, uniq)
    top = np.array(shape, dtype=np.float64) - 1
    v = vertices.astype(np.float64)
    on_face = np.concatenate((v == 0, v == top[None]), axis=1)           # [V, 6]
    same_face = (on_face[d[lonely, 0]] & on_face[d[lonely, 1]]).any(axis=1)
    n_open, bad = int(same_face.sum()), int((~same_face).sum())
    undirected = np.unique(np.minimum(d[:, 0], d[:, 1]) * V + np.maximum(d[:, 0], d[:, 1])).shape[0]
    return undirected, n_open, bad, repeated


def check_mesh(occ, level, vertices, triangles, strict_inside=True):
    """The table-independent checks of this module's docstring.  -> dict(V, F, E, open, bad, repeated)."""
    occ = np.ascontiguousarray(occ, dtype=np.float32)
    X, Y, Z = occ.shape
    assert not bool((occ == np.float32(level)).any()), "choose inputs with no sample on the level"
    cross = crossings(occ, level)
    V, F = int(vertices.shape[0]), int(triangles.shape[0])
    assert vertices.dtype == np.float32 and triangles.dtype == np.int32
    assert V == int(cross.sum()), (V, int(cross.sum()))
    if V == 0:
        assert F == 0
        return dict(V=0, F=0, E=0, open=0, bad=0, repeated=0)
    x, y, z, axis = (a.reshape(-1)[cross.reshape(-1)] for a in np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), np.arange(3), indexing="ij"))
    own = np.stack((x, y, z), axis=1)
    rows = np.arange(V)
    other = np.ones((V, 3), dtype=bool)
    other[rows, axis] = False
    assert bool((vertices[other] == own[other]).all())                   # two integer coordinates: the owner's
    c, i = vertices[rows, axis].astype(np.float64), own[rows, axis].astype(np.float64)
    assert bool(((c >= i) & (c <= i + 1)).all())
    if strict_inside:
        assert bool(((c > i) & (c < i + 1)).all())
    va = occ[x, y, z].astype(np.float64)
    vb = occ[x + (axis == 0), y + (axis == 1), z + (axis == 2)].astype(np.float64)
    err = np.abs(va + (c - i) * (vb - va) - float(np.float32(level)))
    assert bool((err <= 2.0 ** -23 * (i + 2) * np.abs(vb - va)).all()), float((err / np.abs(vb - va)).max())
    assert bool((triangles >= 0).all()) and bool((triangles < V).all())
    assert np.unique(triangles).shape[0] == V                            # no vertex unreferenced
    t = triangles
    assert not bool(((t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 0] == t[:, 2])).any())
    E, n_open, bad, repeated = edge_balance(vertices, triangles, occ.shape)
    assert repeated == 0 and bad == 0, (repeated, bad)
    return dict(V=V, F=F, E=E, open=n_open, bad=bad, repeated=repeated)


# ---- inputs ----
CENTRE = (11.3, 11.7, 11.1)
SPHERE_RADIUS, TORUS_MAJOR, TORUS_MINOR = 8.2, 7.1, 3.05


def _grid(shape):
    return np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")


def sphere(n=24):
    x, y, z = _grid((n, n, n))
    d = np.sqrt((x - CENTRE[0]) ** 2 + (y - CENTRE[1]) ** 2 + (z - CENTRE[2]) ** 2)
    return (SPHERE_RADIUS - d).astype(np.float32)


def torus(n=24):
    x, y, z = _grid((n, n, n))
    q = np.sqrt((x - CENTRE[0]) ** 2 + (y - CENTRE[1]) ** 2) - TORUS_MAJOR
    return (TORUS_MINOR - np.sqrt(q * q + (z - CENTRE[2]) ** 2)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def noise_pair():
    """default_rng(0): the 24^3 draw, then the next 20^3 draw with its outer layer of samples set to 0 (a closed mesh)."""
    rng = np.random.default_rng(0)
    a = rng.random((24, 24, 24)).astype(np.float32)
    b = rng.random((20, 20, 20)).astype(np.float32)
    c = np.zeros_like(b)
    c[1:-1, 1:-1, 1:-1] = b[1:-1, 1:-1, 1:-1]
    return a, c


def shaped_noise(shape, seed):
    """Uniform noise in [0, 1) of any shape, level 0.5."""
    return np.random.default_rng(seed).random(shape).astype(np.float32)


def max_face_only(shape=(6, 5, 7)):
    """Inside only in the far corner sample's three lines: every crossing is an edge on a maximum face of the grid."""
    occ = np.zeros(shape, dtype=np.float32)
    occ[-1, -1, :] = 1.0
    occ[-1, :, -1] = 1.0
    occ[:, -1, -1] = 1.0
    return occ
