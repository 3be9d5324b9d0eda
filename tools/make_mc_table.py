"""Generates open-diffusiongs_amd/csrc/mc_table.h, the marching-cubes case table of csrc/mesh.hip.  This file is the specification of
the table: nothing in it is copied from a published table (it cannot be compared with PyMCubes' triangle for triangle).

    corner k of a cell sits at (dx, dy, dz) = (k >> 2 & 1, k >> 1 & 1, k & 1) from the cell's minimum sample
    case        = sum of inside(k) << k,  inside = occ > level
    edge e      = 4 * axis + r: the cube edge that runs one step along +axis from the owner corner
                  axis 0: owner (0, r >> 1, r & 1);  axis 1: owner (r >> 1, 0, r & 1);  axis 2: owner (r >> 1, r & 1, 0)
    face walk   every cube face's four corners counter-clockwise as seen from outside the cube.  Every maximal run of inside corners is cut
                off by ONE directed segment, from the face edge that leaves the run (inside -> outside) to the one that enters it
                (outside -> inside); four inside corners: no segment.  Two diagonal inside corners are cut off one by one.  The rule reads
                only the face's four signs, so the two cells sharing a face put the same segments on it: the mesh is watertight.
    loops       a crossed edge is the exit of one of its two faces and the entry of the other, so the segments chain into closed
                directed loops over the crossed edges.  Loops are ordered by their smallest edge and start at it.
    triangles   a loop of n edges becomes n - 2 triangles: the first triangulation, in the enumeration of `triangulations`, none of whose
                diagonals lies in a cube face (its two cube edges share a face but are no neighbours in the loop) -- such a diagonal
                would coincide with a diagonal of the neighbouring cell's and give a mesh edge used by four triangles.  Exists for
                all 256 cases (asserted).
    winding     the reverse of the loop direction: normals point from inside to outside, a blob's signed volume is positive (asserted
                here for the one-corner cases).

    python tools/make_mc_table.py            writes the header
    python tools/make_mc_table.py --check    exit status 1 if the committed header differs
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "open-diffusiongs_amd", "csrc", "mc_table.h")
MAX_TRIANGLES = 5


def corner_offset(k):
    return (k >> 2 & 1, k >> 1 & 1, k & 1)


def edge_owner(e):
    """-> (owner corner offset, axis)."""
    axis, r = e >> 2, e & 3
    return ((0, r >> 1, r & 1), (r >> 1, 0, r & 1), (r >> 1, r & 1, 0))[axis], axis


def edge_between(p, q):
    """The edge id of two corner offsets that differ along one axis."""
    axis = [a for a in range(3) if p[a] != q[a]]
    assert len(axis) == 1
    owner = tuple(min(p[a], q[a]) for a in range(3))
    for e in range(12):
        if edge_owner(e) == (owner, axis[0]):
            return e
    raise AssertionError((p, q))


def edge_faces(e):
    """The two cube faces (axis, side) an edge lies in."""
    owner, axis = edge_owner(e)
    return {(b, owner[b]) for b in range(3) if b != axis}


def face_corners(axis, side):
    """Counter-clockwise as seen from outside: (u, v) with e_u x e_v = e_axis walks (0,0) (1,0) (1,1) (0,1) around +e_axis."""
    u, v = (axis + 1) % 3, (axis + 2) % 3
    walk = [(0, 0), (1, 0), (1, 1), (0, 1)]
    if side == 0:                                      # outward normal -e_axis: the other way round
        walk = walk[::-1]
    out = []
    for cu, cv in walk:
        p = [0, 0, 0]
        p[axis], p[u], p[v] = side, cu, cv
        out.append(tuple(p))
    return out


def segments(case):
    """-> {exit edge: entry edge} over all six faces."""
    inside = lambda p: bool(case >> (p[0] * 4 + p[1] * 2 + p[2]) & 1)
    nxt = {}
    for axis in range(3):
        for side in range(2):
            c = face_corners(axis, side)
            flags = [inside(p) for p in c]
            if all(flags) or not any(flags):
                continue
            for i in range(4):
                if flags[i] and not flags[(i + 1) % 4]:                 # the walk leaves a run after corner i
                    j = i
                    while flags[(j - 1) % 4]:
                        j = (j - 1) % 4                                 # first corner of the run
                    leave = edge_between(c[i], c[(i + 1) % 4])
                    enter = edge_between(c[(j - 1) % 4], c[j])
                    assert leave not in nxt
                    nxt[leave] = enter
    return nxt


def loops(case):
    nxt = segments(case)
    assert sorted(nxt) == sorted(nxt.values())                          # every crossed edge leaves one face and enters the other
    inside = lambda p: bool(case >> (p[0] * 4 + p[1] * 2 + p[2]) & 1)
    crossed = []
    for e in range(12):
        owner, axis = edge_owner(e)
        far = tuple(owner[a] + (a == axis) for a in range(3))
        if inside(owner) != inside(far):
            crossed.append(e)
    assert sorted(nxt) == crossed
    out, seen = [], set()
    for e in crossed:                                                   # ascending: a loop starts at its smallest edge
        if e in seen:
            continue
        loop = [e]
        seen.add(e)
        while nxt[loop[-1]] != e:
            loop.append(nxt[loop[-1]])
            seen.add(loop[-1])
        assert len(loop) >= 3
        out.append(loop)
    return out


def triangulations(i, j):
    """All triangulations of the polygon of positions i..j (j - i >= 2) as lists of (a, b, c), a < b < c: the triangle on the side
    (i, j) takes its apex k = i + 1 .. j - 1 in ascending order, then the left part before the right part."""
    if j - i < 2:
        yield []
        return
    for k in range(i + 1, j):
        for left in triangulations(i, k):
            for right in triangulations(k, j):
                yield [(i, k, j)] + left + right


def in_face_diagonals(loop, tris):
    n, bad = len(loop), 0
    for t in tris:
        for a, b in ((t[0], t[1]), (t[1], t[2]), (t[0], t[2])):
            if (b - a) % n in (1, n - 1):
                continue                                                # a side of the loop
            bad += bool(edge_faces(loop[a]) & edge_faces(loop[b]))
    return bad


def case_triangles(case):
    out = []
    for loop in loops(case):
        for tris in triangulations(0, len(loop) - 1):
            if in_face_diagonals(loop, tris) == 0:
                break
        else:
            raise AssertionError(f"case {case}: every triangulation of {loop} has a diagonal in a cube face")
        out += [(loop[a], loop[c], loop[b]) for a, b, c in tris]        # reversed: normals from inside to outside
    assert len(out) <= MAX_TRIANGLES
    return out


def edge_midpoint(e):
    owner, axis = edge_owner(e)
    return tuple(owner[a] + 0.5 * (a == axis) for a in range(3))


def table():
    """-> list of 256 lists of (e0, e1, e2)."""
    t = [case_triangles(c) for c in range(256)]
    for k in range(8):                                                  # one inside corner: the normal points away from it
        (tri,) = t[1 << k]
        p = [edge_midpoint(e) for e in tri]
        u, v = [p[1][a] - p[0][a] for a in range(3)], [p[2][a] - p[0][a] for a in range(3)]
        nrm = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
        away = [p[0][a] - corner_offset(k)[a] for a in range(3)]
        assert sum(nrm[a] * away[a] for a in range(3)) > 0, k
    return t


def packed(t):
    """One 64-bit word per case: nibble 3 i + j = edge j of triangle i, nibble 15 = the number of triangles."""
    words = []
    for tris in t:
        w = len(tris) << 60
        for i, tri in enumerate(tris):
            for j, e in enumerate(tri):
                w |= e << 4 * (3 * i + j)
        words.append(w)
    return words


def header_text():
    words = packed(table())
    lines = ["// mc_table.h -- the marching-cubes case table of mesh.hip.  GENERATED by tools/make_mc_table.py, which is its specification:",
             "// do not edit.  This is the project's own table, derived from the rule stated there; it was not copied from a published",
             "// one and cannot be compared with PyMCubes' triangle for triangle (that package is not available to the project).  The",
             "// surface's vertices are table-independent and therefore the same; the triangulation of a cell's polygon and the choice",
             "// on ambiguous faces may differ.",
             "//   DGS_MC_TABLE[case]: nibble 3 i + j = edge j of triangle i (edge = 4 * axis + r, include/dgs_mesh.h), nibble 15 = the",
             f"//   number of triangles (at most {MAX_TRIANGLES}; {sum(w >> 60 for w in words)} over the 256 cases).",
             "#pragma once", "#include <stdint.h>", "", "__constant__ uint64_t DGS_MC_TABLE[256] = {"]
    for i in range(0, 256, 4):
        lines.append("    " + " ".join(f"0x{w:016x}ull," for w in words[i:i + 4]))
    lines += ["};", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    text = header_text()
    if "--check" in sys.argv:
        sys.exit(0 if open(HEADER).read() == text else 1)
    with open(HEADER, "w") as f:
        f.write(text)
    print(HEADER)
