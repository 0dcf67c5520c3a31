"""corner_scenes.mosaic without a GPU: the layouts that put the leaf adjoints' row sums on their global-atomic arms (more than 64 and more than 255
shapes, a material table too large for the scene description), the hidden shape that no ray reaches — the float64 restatement (tests/ref_path.py)
gives the same image and texture gradient with and without it, array for array — and which rows receive samples on the film the GPU tests
(tests/test_leaf_arms_gpu.py) render: corner_scenes.MOSAIC_FILM, MOSAIC_SPP and MOSAIC_TEX, which both files take, so that a scene too sparse to
exercise the high rows fails here first."""
import numpy as np
import pytest

from fireflies_amd import _abi, scene_desc, scenes
from tests import corner_scenes as cs
from tests import ref_path as rp
from tests.support import world_arrays

FILM, SPP, TEX = cs.MOSAIC_FILM, cs.MOSAIC_SPP, cs.MOSAIC_TEX  # the GPU tests' film (W, H), samples per pixel and projector texture size
SEED = 5


def _desc(sc, shadows=True):
    rows = scenes.material_rows(sc)
    stride = 3 if rows is None else scenes.MAT_STRIDE
    return scene_desc.scene_desc(sc, tex_channels=1, shadows=shadows, mat_stride=stride), (world_arrays(sc)[3] if rows is None else rows)


@pytest.mark.parametrize("S,hidden", [(64, False), (64, True), (255, False), (255, True), (300, False)])
@pytest.mark.parametrize("lambert", [False, True])
def test_layout_is_a_device_table_on_the_arm_it_names(S, hidden, lambert):
    sc = cs.mosaic(S, hidden=hidden, lambert=lambert)
    n = S + int(hidden)
    assert len(sc.meshes) == n and sc.meshes[-1].name == ("mesh-Hidden" if hidden else "mesh-Cube")
    assert [m.name for m in sc.meshes[S - 3:S]] == ["mesh-WallX", "mesh-WallY", "mesh-Cube"]
    assert len({m.material for m in sc.meshes}) == n
    m_ = int(np.ceil(np.sqrt(S - 3)))
    assert sc.n_tris == 2 * m_ * m_ + 2 + 2 + 12 + 2 * int(hidden)  # (every cell of the grid, the walls, the cube)
    assert all(mesh.tris.shape[0] == 2 for mesh in sc.meshes[:S - 4]) and sc.meshes[S - 4].tris.shape[0] == 2 * (m_ * m_ - (S - 4))
    sd, rows = _desc(sc)
    stride = 3 if lambert else scenes.MAT_STRIDE
    assert sd.n_shapes == n and rows.shape == (n, stride) and (int(sd.mat_stride) or 3) == stride
    # the rows do not fit ffx_scene_desc.mat_h: the kernels read a device table
    assert n * stride > _abi.MAX_MAT_H and scene_desc.set_host_materials(sd, rows) is False and sd.n_mat_h == 0
    if not lambert:
        pr = rows[:, scenes.MAT_COLUMN["model"]] != 0
        assert pr[:S - 3].all() and pr[S - 2] and not pr[S - 3] and not pr[S - 1] and (not hidden or pr[S])
        for k, (lo, hi) in {"roughness": (0.2, 0.8), "metallic": (0.0, 0.5)}.items():
            col = rows[pr, scenes.MAT_COLUMN[k]]
            assert (col > lo).all() and (col < hi).all(), k
        assert (rows[pr, scenes.MAT_COLUMN["eta"]] > 1.0).all()
        third = rows[:S - 3:3]
        assert all(((third[:, scenes.MAT_COLUMN[k]] > 0.1) & (third[:, scenes.MAT_COLUMN[k]] < 0.9)).all() for k in ("sheen", "clearcoat", "spec_tint"))


def test_hidden_changes_no_other_index_and_base_textures_take_the_first_cells():
    a, b = cs.mosaic(70, base_tex=4), cs.mosaic(70, base_tex=4, hidden=True)
    ra, rb = scenes.material_rows(a), scenes.material_rows(b)
    assert np.array_equal(ra, rb[:70]) and all(np.array_equal(x.frames, y.frames) and np.array_equal(x.tris, y.tris) for x, y in zip(a.meshes, b.meshes))
    bt = scenes.base_textures(a)
    assert [n for n, _ in bt] == [f"mat-Cell{i}" for i in range(4)] and [list(t.shape[:2]) for _, t in bt] == [list(s) for s in cs.MOSAIC_TEX_SIZES]
    assert list(ra[:5, 15]) == [1.0, 2.0, 3.0, 4.0, 0.0]
    assert scenes.material_rows(cs.mosaic(70, base_tex=2))[:4, 15].tolist() == [1.0, 2.0, 0.0, 0.0]
    assert scenes.material_rows(cs.mosaic(300, lambert=True)) is None  # (the stride-3 table)
    z = b.meshes[-1].frames[0]
    assert (z[:, 2] == np.float32(-0.05)).all() and np.allclose(z[:, :2].mean(0), 1.0) and np.ptp(z[:, 0]) == pytest.approx(0.02, abs=1e-6)


@pytest.mark.parametrize("S", [64, 255])
def test_hidden_shape_is_unseen_by_the_float64_restatement(S):
    """max_depth 4 on a 12 x 12 film: the image and the texture gradient with the hidden shape are the arrays without it, entry for entry — no camera,
    shadow or bounce ray reaches it, so every sample's arithmetic is the same"""
    out = []
    for hidden in (False, True):
        sc = cs.mosaic(S, base_tex=2, hidden=hidden, W=12, H=12, tex=16)
        sd, rows = _desc(sc)
        world = world_arrays(sc)[:3]
        tex = np.random.default_rng(1).random((16, 16, 1))
        gimg = np.random.default_rng(2).uniform(0.5, 1.5, (12, 12, 3))
        out.append((rp.render_fwd(*world, sd, rows, tex, 4, SEED, 4, 2), rp.render_bwd(*world, sd, rows, 4, SEED, gimg, 4, 2)))
    (img, gt), (img_h, gt_h) = out
    print(f"S {S}: max image {img.max():.4g}, sum |gtex| {np.abs(gt).sum():.4g}")
    assert img.max() > 0 and np.abs(gt).sum() > 0
    assert np.array_equal(img, img_h) and np.array_equal(gt, gt_h)


@pytest.mark.parametrize("S,base_tex", [(64, 2), (70, 4), (255, 2), (300, 0)])
def test_rows_receive_samples_on_the_gpu_tests_film(S, base_tex):
    """at FILM, SPP and TEX: at least 90 % of the rows take a primary hit; of the rows with index >= 64 (S > 72) and >= 255 (S > 263) at least 8 take
    one and at least 8 a first bounce's hit; every base-textured cell takes a primary hit"""
    sc = cs.mosaic(S, base_tex=base_tex, W=FILM[0], H=FILM[1], tex=TEX)
    sd, rows = _desc(sc, shadows=False)  # (which shapes the paths meet does not depend on the shadow tests)
    pv = rp.path_vertices(*world_arrays(sc)[:3], sd, rows, SPP, SEED, 3, 3)
    assert len(pv) == 2
    hit = [np.unique(e["shape"]) for _, _, e in pv]
    print(f"S {S}: rows hit at vertex 1 {len(hit[0])} ({len(hit[0]) / S:.3f}), at vertex 2 {len(hit[1])}; with index >= 64: {int((hit[0] >= 64).sum())}, "
          f"{int((hit[1] >= 64).sum())}; with index >= 255: {int((hit[0] >= 255).sum())}, {int((hit[1] >= 255).sum())}")
    assert len(hit[0]) >= 0.9 * S
    for lo in (64, 255):
        if S > lo + 8:
            assert (hit[0] >= lo).sum() >= 8 and (hit[1] >= lo).sum() >= 8, lo
    assert all(i in hit[0] for i in range(base_tex))
