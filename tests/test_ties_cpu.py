"""The tie fixtures of tests/tie_scenes.py, proved on the CPU oracle: each really produces the exact ties it is meant to, and the
oracle resolves them by the rule (closest hit; at equal t the smaller primitive id, whatever the tree).  tests/test_ties_gpu.py is only
meaningful if every condition here holds, so each is asserted.  CPU only."""
import numpy as np
import pytest

from fireflies_amd import scenes, scene_desc
from tests import tie_scenes as ts
from tests.support import bits, host_tex, oracle_geom


@pytest.mark.parametrize("jitter", [0, 1])
@pytest.mark.parametrize("make", [ts.sheets, ts.sheets_far_from_their_plane, ts.sheets_far_unpadded])
def test_stacked_sheets_tie_on_every_ray_and_the_first_shape_wins(oracle, make, jitter):
    out = []
    for fine_first in (False, True):
        sc = make(fine_first)
        g, _ = oracle_geom(oracle, sc)
        t, shape, prim = g.trace_primary(scene_desc.camera_from_sensor(sc.camera), 3, jitter, seed=5)
        assert (shape == 0).all(), f"fine_first={fine_first}: {(shape != 0).sum()} rays do not return shape 0"  # (100 % hit, the first mesh everywhere)
        assert (prim >= 0).all() and (prim < sc.meshes[0].tris.shape[0]).all()
        out.append(t)
    # the same t bits whichever sheet answers: the ray really ties between the sheets
    np.testing.assert_array_equal(bits(out[0]), bits(out[1]))


@pytest.mark.parametrize("shadows", [True, False])
@pytest.mark.parametrize("make", [ts.sheets, ts.sheets_far_from_their_plane, ts.sheets_far_unpadded])
def test_a_coplanar_second_sheet_leaves_the_image_as_it_was(oracle, make, shadows):
    for fine_first in (False, True):
        sc = make(fine_first)
        imgs = []
        for s in (ts.first_sheet_only(sc), sc):
            g, alb = oracle_geom(oracle, s)
            imgs.append(g.render_fwd(scene_desc.scene_desc(s, shadows=shadows), alb, host_tex(s), 8, seed=3))
        assert imgs[0].min() > 0.01  # (lit everywhere)
        assert np.array_equal(imgs[0], imgs[1]), fine_first


@pytest.mark.parametrize("jitter", [0, 1])
@pytest.mark.parametrize("name", ["colon", "vocalfold"])
def test_duplicated_meshes_leave_every_hit_as_it_was(oracle, name, jitter):
    sc = ts.dup_cases()[name]()
    cam = scene_desc.camera_from_sensor(sc.camera)
    t1, s1, p1 = oracle_geom(oracle, sc)[0].trace_primary(cam, 1, jitter, seed=5)
    t2, s2, p2 = oracle_geom(oracle, ts.duplicated(sc))[0].trace_primary(cam, 1, jitter, seed=5)
    assert (p1 >= 0).mean() > 0.5
    assert (p2 < sc.n_tris).all()
    np.testing.assert_array_equal(bits(t2), bits(t1))
    np.testing.assert_array_equal(p2, p1)
    np.testing.assert_array_equal(s2, s1)


@pytest.mark.parametrize("shadows", [True, False])
@pytest.mark.parametrize("name", ["colon", "vocalfold", "hello"])
def test_duplicated_meshes_leave_the_image_as_it_was(oracle, name, shadows):
    sc = ts.dup_cases()[name]()
    dup = ts.duplicated(sc)
    tex = host_tex(sc)
    imgs = []
    for s in (sc, dup):
        g, alb = oracle_geom(oracle, s)
        imgs.append(g.render_fwd(scene_desc.scene_desc(s, shadows=shadows), alb, tex, 8, seed=3))
    assert imgs[0].max() > 0.01
    assert np.array_equal(imgs[0], imgs[1])


@pytest.mark.parametrize("name", list(ts.seam_cases()))
def test_seams_of_the_stock_scenes_tie_without_jitter_only(oracle, name):
    """relabelling (the triangle order reversed inside every mesh) changes the geometric pick of exactly the rays the id order decided"""
    sc = ts.seam_cases()[name]()
    rev = ts.reversed_tris(sc)
    cam = scene_desc.camera_from_sensor(sc.camera)
    g, gr = oracle_geom(oracle, sc)[0], oracle_geom(oracle, rev)[0]
    t, s, p = g.trace_primary(cam, 1, 0, 0)
    tr, sr, pr = gr.trace_primary(cam, 1, 0, 0)
    np.testing.assert_array_equal(bits(tr), bits(t))
    np.testing.assert_array_equal(sr, s)
    tied = ts.map_back(pr, sc) != p
    assert tied.sum() >= 5, f"{name}: only {tied.sum()} tied rays of {(p >= 0).sum()} hits"
    t, s, p = g.trace_primary(cam, 1, 1, 7)
    tr, sr, pr = gr.trace_primary(cam, 1, 1, 7)
    np.testing.assert_array_equal(bits(tr), bits(t))
    assert (ts.map_back(pr, sc) == p).all()


def test_map_back_inverts_the_relabelling():
    sc = ts.small_vocalfold()
    F = sc.n_tris
    ids = np.arange(-1, F, dtype=np.int32)
    back = ts.map_back(ids, sc)
    assert back[0] == -1 and sorted(back[1:]) == list(range(F))
    _, tris, shape, off, *_ = scenes.flatten(sc)
    _, tris_r, shape_r, *_ = scenes.flatten(ts.reversed_tris(sc))
    np.testing.assert_array_equal(tris_r[ids[1:]], tris[back[1:]])
    np.testing.assert_array_equal(shape_r[ids[1:]], shape[back[1:]])


@pytest.mark.parametrize("jitter", [0, 1])
def test_coincident_triangles_beyond_the_wide_walks_budget(oracle, jitter):
    sc = ts.budget()
    assert sc.n_tris == 128  # > FFX_WIDE_MAX_WORK = 96 exact tests (fireflies_amd/csrc/ffx_trace.hip)
    t, s, p = oracle_geom(oracle, sc)[0].trace_primary(scene_desc.camera_from_sensor(sc.camera), 3, jitter, seed=2)
    hit = p >= 0
    assert 0.2 < hit.mean() < 0.9
    assert set(np.unique(p[hit])) == {0, 1}


def test_lattice_rays_reference_equals_the_oracle_bit_for_bit(oracle):
    mesh, o, d, ties = ts.lattice()
    t_ref, p_ref, n_tied = ts.tri_hit_all_pairs(mesh.frames[0], mesh.tris, o, d)
    assert (p_ref >= 0).all()
    np.testing.assert_array_equal(n_tied, ties)  # (6 triangles at an interior vertex, 2 on an interior edge)
    assert (ties == 6).sum() == 49 and (ties == 2).sum() > 150
    np.testing.assert_array_equal(t_ref, np.where(d[:, 2] == 4, 1.0, 0.5).astype(np.float32))
    g, _ = oracle_geom(oracle, scenes.SceneData([mesh], None))
    t, s, p = g.trace_rays(o, d)
    np.testing.assert_array_equal(bits(t), bits(t_ref))
    np.testing.assert_array_equal(p, p_ref)
    assert (s == 0).all()
