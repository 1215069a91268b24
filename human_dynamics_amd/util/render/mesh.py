"""Closed test meshes for the rasteriser."""
from __future__ import annotations

import numpy as np


def latlong_sphere(n_lon=84, n_rings=82):
    """A closed genus-0 mesh: n_lon * n_rings ring vertices + 2 poles, 2 n_lon n_rings faces.  The defaults give SMPL's
    counts (6 890 vertices, 13 776 faces).  -> verts [V,3] float32 on the unit sphere, faces [F,3] int32 (outward
    counter-clockwise)."""
    th = np.pi * (np.arange(n_rings) + 1) / (n_rings + 1)            # polar angle of each ring
    ph = 2 * np.pi * np.arange(n_lon) / n_lon
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph)[None], np.cos(th)[:, None] * np.ones_like(ph)[None],
                     np.sin(th)[:, None] * np.sin(ph)[None]], -1).reshape(-1, 3)
    verts = np.concatenate([[[0, 1, 0]], ring, [[0, -1, 0]]]).astype(np.float32)
    top, bot = 0, len(verts) - 1

    def vid(r, k):
        return 1 + r * n_lon + (k % n_lon)
    faces = []
    for k in range(n_lon):
        faces.append([top, vid(0, k + 1), vid(0, k)])
    for r in range(n_rings - 1):
        for k in range(n_lon):
            a, b, c, d = vid(r, k), vid(r, k + 1), vid(r + 1, k), vid(r + 1, k + 1)
            faces.append([a, b, d])
            faces.append([a, d, c])
    for k in range(n_lon):
        faces.append([bot, vid(n_rings - 1, k), vid(n_rings - 1, k + 1)])
    return verts, np.asarray(faces, np.int32)


def deformed_sphere(seed=0, scale=(0.35, 0.8, 0.25), n_lon=84, n_rings=82):
    """The SMPL-sized sphere smoothly deformed into a person-like ellipsoid with low-frequency bumps (metres-ish units,
    like SMPL's vertices).  n_lon, n_rings: latlong_sphere's (14, 12: 170 vertices, for tests that need a mesh, not its size)."""
    v, f = latlong_sphere(n_lon, n_rings)
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.05, 0.15, 3)
    k = rng.integers(1, 4, 3)
    bump = 1 + a[0] * np.sin(k[0] * 3 * v[:, 1]) + a[1] * np.cos(k[1] * 2 * v[:, 0]) + a[2] * np.sin(k[2] * (v[:, 2] + v[:, 1]))
    v = v * bump[:, None] * np.asarray(scale, np.float32)[None]
    return v.astype(np.float32), f
