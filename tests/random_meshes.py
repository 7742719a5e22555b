"""The random mesh family of the seeded sweeps (tests/test_hip_fuzz.py, tests/test_hip_operator_fuzz.py)
-- test infrastructure, a plain module.

Delaunay and structured meshes of random size with random element removal (open fans, several
fans per vertex, isolated vertices), random orientation flips, rotated local numbering, shuffled
or Morton vertex order, shuffled element order.  One mesh in ten is large (many tiles).

The generator consumes its `rng` in a FIXED order: a seed names a mesh, and the sweeps' records of
what they exercised depend on it (tests/test_operator_reference.py pins a few seeds by hash)."""

import numpy as np


def random_mesh(rng):
    """(vertices (N, 2) float64, triangles (E, 3) int32) drawn from `rng`."""
    from pytorch_fem_solver_amd import meshgen

    big = rng.random() < 0.1  # now and then a mesh of many tiles
    if rng.random() < 0.5:
        mesh = meshgen.unit_square(int(rng.integers(2, 200 if big else 60)), float(rng.uniform(0.0, 0.3)),
                                   int(rng.integers(1 << 30)))
    else:
        mesh = meshgen.delaunay_square(int(rng.integers(30, 40000 if big else 4000)), int(rng.integers(1 << 30)))
    verts, tris = mesh["vertices"].copy(), mesh["triangles"].copy()
    if rng.random() < 0.5:  # holes: open fans, several fans per vertex, isolated vertices
        keep = rng.random(tris.shape[0]) >= rng.uniform(0.02, 0.3)
        if keep.sum() >= 1:
            tris = tris[keep]
    if rng.random() < 0.5:  # stored orientation
        flip = rng.random(tris.shape[0]) < rng.uniform(0.05, 0.6)
        tris[flip] = tris[flip][:, [0, 2, 1]]
    if rng.random() < 0.5:  # rotate the local numbering of elements
        shift = rng.integers(0, 3, size=tris.shape[0])
        tris = np.stack([tris[np.arange(tris.shape[0]), (shift + j) % 3] for j in range(3)], axis=1)
    renumber = rng.random()
    if renumber < 0.7:  # numbering without locality (< 0.35) or along a Morton curve
        perm = rng.permutation(verts.shape[0]) if renumber < 0.35 else meshgen.morton_order(verts)
        inv = np.empty_like(perm)
        inv[perm] = np.arange(perm.size)
        verts, tris = verts[perm], inv[tris].astype(np.int32)
    if rng.random() < 0.4:
        tris = tris[rng.permutation(tris.shape[0])]
    return verts, np.ascontiguousarray(tris.astype(np.int32))


def has_elements(tris, n_verts):
    """(N,) bool: the vertices that some element touches (the others are isolated: empty rows)."""
    return np.bincount(np.asarray(tris).reshape(-1), minlength=n_verts) > 0
