"""The rasteriser's host side (include/hmmr_hip.h: hmmr_render_mesh, csrc/render.hip): the C ABI and its validation with
dummy pointers (nothing is launched), the workspace query, the geometry helpers, face loading, and the basic laws of
the NumPy spec (tests/render_oracle.py) that the GPU tests hold the kernel to.  No GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest

import render_oracle as O
from human_dynamics_amd import _lib

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------------------------------------------- the C ABI
def test_render_symbols_are_bound_and_abi_unchanged():
    lib = _lib.load()
    for name in ("hmmr_render_mesh", "hmmr_render_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.hmmr_abi_version() == 19


def test_render_desc_matches_the_header_field_order():
    hdr = open(os.path.join(os.path.dirname(GOLD), "..", "include", "hmmr_hip.h")).read()
    body = hdr[hdr.index("const float* verts; int64_t ld_verts;"):hdr.index("} hmmr_render_desc_t;")]
    import re
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.replace("\n", " ").split(";"):
        for part in decl.split(","):
            m = re.search(r"\*?\s*([a-z_0-9]+)\s*(\[\d+\])?\s*$", part.strip())
            if m:
                names.append(m.group(1))
    assert names == [f for f, _ in _lib.RenderDesc._fields_]


def test_render_workspace_query():
    lib = _lib.load()
    one = lib.hmmr_render_workspace_bytes(1, 6890, 13776)
    assert one >= 6890 * 16 + 13776 * (8 + 48 + 16)
    big = lib.hmmr_render_workspace_bytes(4096, 6890, 13776)
    assert big == lib.hmmr_render_workspace_bytes(64, 6890, 13776)      # frames go in slabs: bounded workspace
    assert one < big < 64 * 6890 * 16 + 64 * 13776 * 80 + 4096
    for bad in ((0, 10, 10), (4097, 10, 10), (1, 0, 10), (1, 10, 0), (1, 10, 65537)):
        assert lib.hmmr_render_workspace_bytes(*bad) == 0


def _desc(n=2, size=64):
    d = _lib.RenderDesc()
    d.verts, d.ld_verts, d.cams, d.ld_cam = 0x1000, 30, 0x2000, 3
    d.faces, d.rgb, d.ws = 0x3000, 0x4000, 0x5000
    d.n, d.nv, d.nf, d.size = n, 10, 8, size
    d.out_h = d.out_w = size
    d.ws_bytes = _lib.load().hmmr_render_workspace_bytes(n, 10, 8)
    return d


@pytest.mark.parametrize("field,value,msg", [
    ("verts", None, b"NULL operand"), ("faces", None, b"NULL operand"), ("rgb", None, b"NULL operand"),
    ("ws", None, b"NULL operand"), ("n", 0, b"n = 0"), ("n", 4097, b"n = 4097"), ("size", 15, b"size = 15"),
    ("size", 1025, b"size = 1025"), ("nf", 0, b"nf = 0"), ("nf", 65537, b"nf = 65537"), ("nv", 2, b"nv = 2"),
    ("ld_verts", 29, b"row strides"), ("ld_cam", 2, b"row strides"), ("out_h", 65, b"output"), ("out_w", 0, b"output"),
    ("bg_mode", 3, b"bg_mode"), ("bg_mode", 1, b"without bg_image"), ("ws_bytes", 100, b"workspace"),
])
def test_render_mesh_validates_before_any_launch(field, value, msg):
    lib = _lib.load()
    d = _desc()
    setattr(d, field, value)
    assert lib.hmmr_render_mesh(C.byref(d), None) == -1
    assert msg in lib.hmmr_last_error(), lib.hmmr_last_error()
    assert lib.hmmr_render_mesh(None, None) == -1


def test_render_mesh_refuses_a_frame_background_without_its_size():
    lib = _lib.load()
    d = _desc()
    d.bg_mode, d.bg_image = 2, 0x6000
    assert lib.hmmr_render_mesh(C.byref(d), None) == -1 and b"frame size" in lib.hmmr_last_error()
    d = _desc()
    d.face_colors, d.ld_face_colors = 0x6000, 5
    assert lib.hmmr_render_mesh(C.byref(d), None) == -1 and b"face_colors" in lib.hmmr_last_error()


# ------------------------------------------------------------------------------------------------ python helpers
def test_orig_output_size_and_geometry_against_the_reference_fixture():
    from human_dynamics_amd.util.render.video import orig_output_size
    g = np.load(os.path.join(GOLD, "reference_render.npz"))
    for (h, w, max_img), (oh, ow) in zip(g["orig_params"], g["orig_out_hw"]):
        hh, ww, S = orig_output_size((h, w), max_img)
        assert (hh, ww) == (oh, ow) and S == max(oh, ow)


def test_faces_load_from_npy_and_from_an_smpl_pickle(tmp_path):
    import published_formats as pf
    from human_dynamics_amd.util.render.nmr_renderer import load_faces
    from human_dynamics_amd.util.render.mesh import latlong_sphere
    _, f = latlong_sphere(12, 10)
    np.save(tmp_path / "faces.npy", f.astype(np.int64))
    assert np.array_equal(load_faces(str(tmp_path / "faces.npy")), f)
    p = pf.Py2Pickle()
    p.dict_({"f": f.astype(np.uint32), "v_template": pf.Chumpy(np.zeros((122, 3)))})
    (tmp_path / "m.pkl").write_bytes(p.done())
    got = load_faces(str(tmp_path / "m.pkl"))
    assert got.dtype == np.int32 and np.array_equal(got, f)


def test_vis_renderer_refuses_large_textures_and_bad_faces():
    from human_dynamics_amd.util.render.nmr_renderer import VisRenderer
    from human_dynamics_amd.util.render.raster import MeshFaces
    f = np.array([[0, 1, 2]], np.int32)
    with pytest.raises(NotImplementedError):
        VisRenderer(64, faces=f, t_size=2)
    r = VisRenderer(64, faces=f, device="cpu")
    r.renderer.image_size = 96                      # visualize_img_orig assigns it
    assert r.renderer.image_size == 96 and r.renderer.background_color == [1, 1, 1.]
    assert r.renderer.light_direction == [1, .5, -1]
    with pytest.raises(ValueError):
        MeshFaces(np.array([[0, 1, -1]]))
    with pytest.raises(ValueError):
        MeshFaces(np.zeros((3, 4), np.int32))
    rgba = r.make_alpha(np.full((2, 2, 3), 7.9), np.full((2, 2, 1), 0.75))
    assert rgba.shape == (2, 2, 4) and rgba[0, 0, 0] == 7 and rgba[0, 0, 3] == 191


def test_rodrigues_keeps_the_tiny_cosine():
    from human_dynamics_amd.util.render.raster import rodrigues
    R = rodrigues(90, 'y')
    assert R[0, 0] == np.cos(np.pi / 2) and R[0, 0] != 0
    assert np.allclose(R, [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], atol=1e-15)
    assert np.allclose(O.rodrigues(90, 'y'), R)


def test_sphere_has_smpl_counts_and_is_closed():
    from collections import Counter
    from human_dynamics_amd.util.render.mesh import latlong_sphere
    v, f = latlong_sphere()
    assert v.shape == (6890, 3) and f.shape == (13776, 3)
    e = Counter(tuple(sorted((int(t[i]), int(t[(i + 1) % 3])))) for t in f for i in range(3))
    assert set(e.values()) == {2}


# ------------------------------------------------------------------------------------------------ the spec's laws
def _tri(pts, z=0.0):
    """projected vertices from unflipped (x, y): p = (x, -y, z)"""
    p = np.array([[x, -y, z] for x, y in pts], np.float32)
    return p


def test_single_triangle_covers_what_its_edge_functions_say():
    S = 16
    p = _tri([(-0.6, -0.5), (0.7, -0.2), (0.1, 0.8)])
    idx, amb = O.rasterize(p, np.array([[0, 1, 2]]), S)
    S2 = 2 * S
    c = (2 * np.arange(S2) + 1 - S2) / S2
    u, v = np.meshgrid(c, c)
    q = p[:, :2].astype(np.float64) * [1, -1]
    inside = np.ones_like(u, bool)
    area = (q[1, 0] - q[0, 0]) * (q[2, 1] - q[0, 1]) - (q[1, 1] - q[0, 1]) * (q[2, 0] - q[0, 0])
    for i in range(3):
        a, b = q[(i + 1) % 3], q[(i + 2) % 3]
        e = (a[0] - u) * (b[1] - v) - (a[1] - v) * (b[0] - u)
        inside &= e * np.sign(area) >= 0
    assert np.array_equal(idx >= 0, inside)
    assert inside.sum() > 100 and not amb[inside].all()


def test_both_windings_shade_with_the_viewer_facing_normal():
    p = _tri([(-0.5, -0.5), (0.5, -0.5), (0.0, 0.5)])
    p[2, 2] = 0.3                                            # tilt it so that n . d depends on the normal's sign
    c1 = O.shade(p, np.array([[0, 1, 2]]))
    c2 = O.shade(p, np.array([[2, 1, 0]]))
    assert np.allclose(c1, c2)
    n = np.cross(p[0] - p[1], p[2] - p[1]).astype(np.float64)
    n = n if n[2] <= 0 else -n
    n /= np.linalg.norm(n)
    exp = np.asarray(O.COLORS['blue']) * (0.7 + 0.3 * max(0.0, n @ [1, .5, -1]))
    assert np.allclose(c1[0], exp)
    idx1, _ = O.rasterize(p, np.array([[0, 1, 2]]), 16)
    idx2, _ = O.rasterize(p, np.array([[2, 1, 0]]), 16)
    assert np.array_equal(idx1, idx2)                         # fill_back: drawn whatever the winding


def test_nearer_of_two_overlapping_triangles_wins_and_a_tie_goes_to_the_lower_index():
    a = _tri([(-0.8, -0.8), (0.8, -0.8), (0.0, 0.8)], z=0.5)
    b = _tri([(-0.7, -0.7), (0.7, -0.7), (0.0, 0.7)], z=-0.5)   # nearer (z' smaller)
    p = np.concatenate([a, b])
    idx, amb = O.rasterize(p, np.array([[0, 1, 2], [3, 4, 5]]), 16)
    inner = (idx >= 0) & ~amb
    assert (idx[inner] == 1).sum() > 50 and (idx[inner] == 0).sum() > 0     # the rim of the far one shows
    idx2, _ = O.rasterize(p, np.array([[3, 4, 5], [0, 1, 2]]), 16)
    assert np.array_equal(idx2[inner], 1 - idx[inner])                     # order does not decide depth
    same = np.concatenate([a, a])
    idx3, amb3 = O.rasterize(same, np.array([[0, 1, 2], [3, 4, 5]]), 16)
    assert set(np.unique(idx3)) == {-1, 0} and amb3[idx3 == 0].all()       # an exact tie: lower index, flagged


def test_the_near_plane_cuts():
    # z' = z + 2.732: from z' = 0.05 on the left to z' = 2.0 on the right, so the left part is in front of near = 0.1
    p = np.array([[-0.9, 0.9, 0.05 - 2.7320508], [0.9, 0.9, 2.0 - 2.7320508], [0.9, -0.9, 2.0 - 2.7320508],
                  [-0.9, -0.9, 0.05 - 2.7320508]], np.float32)
    idx, amb = O.rasterize(p, np.array([[0, 1, 2], [0, 2, 3]]), 32)
    cols_drawn = np.nonzero((idx >= 0).any(axis=0))[0]
    # 1/z' is linear in screen space (harmonic depth): z' = 0.1 about half-way, 0.9 * 32 + 31.5 = subpixel 60 on the right
    assert 28 <= cols_drawn.min() <= 36 and cols_drawn.max() == 60


def test_alpha_levels_are_quarters():
    p = _tri([(-0.63, -0.41), (0.77, -0.13), (0.05, 0.71)])
    r = O.render(p, np.array([[0, 1, 2]]), 24)
    assert set(np.unique(r["alpha"])) == {0.0, 0.25, 0.5, 0.75, 1.0}
    assert r["rgb"].dtype == np.uint8 and r["rgb"].shape == (24, 24, 3)
    assert (r["rgb"][r["alpha"] == 0] == 255).all()                         # white background


def test_non_finite_and_zero_area_faces_draw_nothing():
    p = _tri([(-0.5, -0.5), (0.5, -0.5), (0.0, 0.5), (0.2, 0.2)])
    p[3, 0] = np.nan
    idx, _ = O.rasterize(p, np.array([[0, 1, 3], [0, 0, 2], [0, 1, 1]]), 16)
    assert (idx == -1).all()
