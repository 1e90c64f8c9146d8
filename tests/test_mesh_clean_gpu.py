"""The mesh cleaning kernels (csrc/mesh_clean.hip) on the GPU: adjacency (CSR and fixed flags), component labels and stats, the
removed mesh and the smoothed vertices bit-equal to the numpy restatement of tests/test_mesh_clean.py on the hand cases, random
soups (non-manifold edges, a vertex of more than 1000 faces: the long-row path), a strip of 10^5 triangles and the floater
scenes of tests/mesh_clean_scene.py; face-order invariance; the spike a floater leaves in the mesh DSM, gone after cleaning; the
PLY of predict_and_fuse(mesh={..., clean steps}) equal to the one python -m deep3d_aerial_amd.mesh --clean writes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_clean_scene as CS
import mesh_scene as MS
import test_mesh_clean as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _dev(v, f):
    return torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(f, np.int32)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _check_all(v, f, min_faces, spurious, smooth=2, lam=0.5):
    """Every pass of the kernels against the restatement; returns the GPU's cleaned mesh."""
    from deep3d_aerial_amd import mesh

    n = len(v)
    V, F = _dev(v, f)
    offset, nbr, fixed = mesh.adjacency(F, n)
    w_off, w_nbr, w_fixed = T.adjacency_numpy(n, f)
    assert np.array_equal(offset.cpu().numpy(), w_off)
    assert np.array_equal(nbr[:int(offset[-1])].cpu().numpy(), w_nbr)
    assert np.array_equal(fixed.cpu().numpy(), w_fixed)
    labels, rounds = mesh.components(F, n)
    w_label = T.components_numpy(n, f)
    assert np.array_equal(labels.cpu().numpy(), w_label) and rounds >= 1
    st = mesh.component_stats(V, F, labels)
    count, box, diag, gbox, gdiag = T.stats_numpy(v, f, w_label)
    assert np.array_equal(st["face_count"].cpu().numpy(), count)
    assert np.array_equal(st["box"].cpu().numpy(), box, equal_nan=True)
    assert np.array_equal(st["diag"].cpu().numpy(), diag, equal_nan=True)
    assert np.array_equal(st["global_box"].cpu().numpy(), gbox) and float(st["global_diag"][0]) == gdiag
    info = {}
    Vr, Fr = mesh.remove_components(V, F, min_faces, spurious, info=info)
    wv, wf = T.remove_numpy(v, f, min_faces, spurious)
    assert np.array_equal(_bits(Vr.cpu().numpy()), _bits(wv)) and np.array_equal(Fr.cpu().numpy(), wf)
    assert info["faces_removed"] == len(f) - len(wf)
    Vs = mesh.smooth_vertices(V, F, smooth, lam)
    assert np.array_equal(_bits(Vs.cpu().numpy()), _bits(T.smooth_numpy(v, f, smooth, lam)))
    Vc, Fc = mesh.clean(V, F, min_faces, spurious, smooth, lam)
    cv, cf = T.clean_numpy(v, f, min_faces, spurious, smooth, lam)
    assert np.array_equal(_bits(Vc.cpu().numpy()), _bits(cv)) and np.array_equal(Fc.cpu().numpy(), cf)
    return Vc.cpu().numpy(), Fc.cpu().numpy()


@pytest.mark.parametrize("name", sorted(T.HAND))
def test_hand_cases_are_bit_equal_to_numpy(name):
    v, f = T.HAND[name]
    _check_all(v, f, 5, 5.0, smooth=3, lam=0.5)
    _check_all(v, f, 0, 20.0, smooth=1, lam=1.0)


def _soup(seed, n, m, hub_faces=0):
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal((n, 3)) * rng.uniform(0.1, 10, (n, 1))).astype(np.float32)
    f = rng.integers(0, n, (m, 3)).astype(np.int32)
    f[: m // 10, 1] = f[: m // 10, 0]               # repeated indices
    f[m // 10: m // 5] = f[m // 10: m // 5][:, ::-1]   # both windings
    if hub_faces:
        f[-hub_faces:, 0] = 7                        # a vertex of more than 1000 faces: its row takes the long path
    f[m // 5: m // 5 + 40] = f[m // 5 + 40: m // 5 + 80]   # duplicated faces: edges of multiplicity 2 .. 4
    return v, f


@pytest.mark.parametrize("seed,n,m,hub", [(0, 50, 200, 0), (1, 3000, 2000, 0), (2, 20000, 30000, 1500), (3, 5000, 4000, 2500)])
def test_random_soups_are_bit_equal_to_numpy(seed, n, m, hub):
    v, f = _soup(seed, n, m, hub)
    if hub:
        assert (np.bincount(f.ravel(), minlength=n) > 1000).any()
    _check_all(v, f, 3, 50.0, smooth=2, lam=0.5)


def test_strip_of_100000_triangles():
    """A strip of 10^5 triangles under a random vertex numbering: one long chain for the component rounds."""
    k = 50001
    rng = np.random.default_rng(5)
    x = np.arange(k, dtype=np.float32)
    v = np.concatenate([np.stack([x, np.zeros(k), np.sin(x / 50)], 1), np.stack([x, np.ones(k), np.cos(x / 70)], 1)]).astype(np.float32)
    i = np.arange(k - 1)
    f = np.concatenate([np.stack([i, i + 1, k + i], 1), np.stack([i + 1, k + i + 1, k + i], 1)]).astype(np.int64)
    perm = rng.permutation(2 * k)
    v2 = np.empty_like(v)
    v2[perm] = v
    f2 = perm[f].astype(np.int32)
    # plus a short strip far away that both rules remove
    v3 = np.concatenate([v2, np.float32([[0, 5, 0], [1, 5, 0], [0, 6, 0], [1, 6, 0]])])
    f3 = np.concatenate([f2, np.int32([[2 * k, 2 * k + 1, 2 * k + 2], [2 * k + 1, 2 * k + 3, 2 * k + 2]])])
    assert len(f3) > 100000
    Vc, Fc = _check_all(v3, f3, 10, 20.0, smooth=2)
    assert len(Fc) == len(f2)
    from deep3d_aerial_amd import mesh

    _, rounds = mesh.components(_dev(v3, f3)[1], len(v3))
    print("strip rounds", rounds)


def test_face_order_does_not_change_the_result():
    from deep3d_aerial_amd import mesh

    v, f = _soup(6, 4000, 6000, 1200)
    p = np.random.default_rng(7).permutation(len(f))
    V, F = _dev(v, f)
    _, Fp = _dev(v, f[p])
    a = mesh.adjacency(F, len(v))
    b = mesh.adjacency(Fp, len(v))
    for x, y in zip(a, b):
        assert torch.equal(x[:int(a[0][-1])] if x.dtype == torch.int32 else x, y[:int(a[0][-1])] if y.dtype == torch.int32 else y)
    V1, F1 = mesh.clean(V, F, 3, 30.0, 2)
    V2, F2 = mesh.clean(V, Fp, 3, 30.0, 2)
    assert torch.equal(V1.view(torch.int32), V2.view(torch.int32))
    assert sorted(map(tuple, F1.cpu().numpy().tolist())) == sorted(map(tuple, F2.cpu().numpy().tolist()))


def test_all_steps_off_return_the_input_and_errors():
    from deep3d_aerial_amd import mesh

    v, f = T.HAND["unreferenced"]
    V, F = _dev(v, f)
    V2, F2 = mesh.clean(V, F)
    assert V2 is V and F2 is F
    with pytest.raises(ValueError, match="outside"):
        mesh.clean(V, F + 3, min_faces=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.clean(V.cpu(), F.cpu(), min_faces=2)
    with pytest.raises(ValueError, match="smooth_lambda"):
        mesh.clean(V, F, smooth=1, smooth_lambda=0.0)
    E = torch.zeros((0, 3), dtype=torch.int32, device="cuda")
    V3, F3 = mesh.clean(V, E, min_faces=2, smooth=1)
    assert V3.shape == (0, 3) and F3.shape == (0, 3)
    V4 = mesh.smooth_vertices(V, E, 2)
    assert torch.equal(V4, V)


def _raw_mesh(views, border, voxel):
    from deep3d_aerial_amd import mesh

    mv = [mesh.MeshView(x["K"], x["E"], torch.from_numpy(x["depth"]).cuda(), torch.from_numpy(x["confidence"]).cuda()) for x in views]
    return mesh.depth_to_mesh(mv, mesh.MeshGrid(border, voxel))


def _floating_pieces(V, F, floaters, voxel):
    """Components whose box lies inside a floater's box grown by four voxels (the TSDF surface reaches below its bottom)."""
    from deep3d_aerial_amd import mesh

    labels, _ = mesh.components(F, V.shape[0])
    st = mesh.component_stats(V, F, labels)
    cnt, box = st["face_count"].cpu().numpy(), st["box"].cpu().numpy()
    found = []
    for x0, x1, y0, y1, z0, z1 in floaters:
        lo = np.array([x0, y0, z0]) - 4 * voxel
        hi = np.array([x1, y1, z1]) + 4 * voxel
        inside = (cnt > 0) & (box[:, :3] >= lo).all(1) & (box[:, 3:] <= hi).all(1)
        found.append(int(inside.sum()))
    return found


def _spikes(V, F, border, voxel, height_near):
    from deep3d_aerial_amd import dsm

    grid = dsm.DsmGrid(border[:4], voxel)
    h = dsm.mesh_to_dsm(V, F, grid).cpu().numpy()
    i, j = np.mgrid[0:grid.height, 0:grid.width]
    x = grid.x_min + (j + 0.5) * voxel
    y = grid.y_max - (i + 0.5) * voxel
    return int((np.nan_to_num(h, nan=-1e9) > height_near(x, y, 1.0) + 1.0).sum())


@pytest.mark.parametrize("seed", [4, 8])
def test_floater_scene_pieces_are_removed_and_the_dsm_spikes_go(seed):
    from deep3d_aerial_amd import mesh

    border, voxel, views, floaters, height_near = CS.floater_scene(seed)
    V, F = _raw_mesh(views, border, voxel)
    v, f = V.cpu().numpy(), F.cpu().numpy()
    assert len(f) > 2000
    assert all(k >= 1 for k in _floating_pieces(V, F, floaters, voxel)), "the raw mesh must hold every floater"
    raw_spikes = _spikes(V, F, border, voxel, height_near)
    assert raw_spikes >= 4, raw_spikes
    for kw in ({"min_faces": 1000}, {"spurious": 5.0}):
        Vc, Fc = _check_all(v, f, kw.get("min_faces", 0), kw.get("spurious", 0.0), smooth=1)
        Vc, Fc = mesh.clean(V, F, **kw)
        assert _floating_pieces(Vc, Fc, floaters, voxel) == [0] * len(floaters)
        assert _spikes(Vc, Fc, border, voxel, height_near) == 0
        assert len(Fc) > 0.9 * len(f)
    Vs = mesh.clean(V, F, smooth=2)[0].cpu().numpy()
    assert np.array_equal(_bits(Vs), _bits(T.smooth_numpy(v, f, 2)))


def test_predict_and_fuse_writes_the_cleaned_mesh_the_cli_writes(tmp_path):
    import pipeline_scene as PS
    from deep3d_aerial_amd import mesh, pipeline

    border, voxel = _pipeline_border(tmp_path)
    scene = PS.SceneViews()
    settings = MS.pipeline_settings(str(tmp_path / "a" / "mesh.ply"), border, voxel)
    settings.update(min_faces=50, spurious=10.0, smooth=1)
    pipeline.predict_and_fuse(PS.SceneModel(scene), scene, str(tmp_path / "a" / "MVS"), checker=PS.checker(), fusion_num=PS.FUSION_NUM,
                              min_geo_consist_num=3, filter_sources=False, mesh=settings)
    views = []
    for i in range(len(scene)):
        it = scene[i]
        views.append(mesh.MeshView(it["outcam"][1, :3, :3], it["outcam"][0], torch.from_numpy(scene.views[i]["depth"]).cuda(),
                                   torch.from_numpy(scene.views[i]["confidence"]).cuda()))
    V, F = mesh.depth_to_mesh(views, mesh.MeshGrid(border, voxel))
    raw = str(tmp_path / "raw.ply")
    mesh.write_ply(raw, V, F)
    out = tmp_path / "cli.ply"
    res = subprocess.run([sys.executable, "-m", "deep3d_aerial_amd.mesh", "--clean", raw, "--out", str(out), "--min_faces", "50",
                          "--spurious", "10", "--smooth", "1"], cwd=ROOT,
                         env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")),
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    assert out.read_bytes() == (tmp_path / "a" / "mesh.ply").read_bytes()
    Vc, Fc = mesh.read_ply(str(out))
    cv, cf = T.clean_numpy(V.cpu().numpy(), F.cpu().numpy(), 50, 10.0, 1)
    assert np.array_equal(_bits(Vc), _bits(cv)) and np.array_equal(Fc, cf) and len(Fc) > 100


def _pipeline_border(tmp_path):
    import test_mesh_gpu as G

    return G._border(tmp_path)
