"""The decimation kernels (csrc/mesh_decimate.hip) on the GPU: face incidence, vertex quadrics, every candidate's target, cost and
key, the threshold, the claims, the winner set and the mesh after each round bit-equal to the numpy restatement of
tests/test_mesh_decimate.py, and whole runs for several targets, on a planar grid, a noisy grid, a closed sphere, a cone whose
apex has 1500 faces, the boxes and sphere scenes of tests/mesh_scene.py meshed on the GPU and random soups; the properties the
rule promises, checked with mesh.adjacency; the comparison with a coarser voxel at equal face count; the PLY of
predict_and_fuse(mesh={..., "decimate": R}) equal to the one python -m deep3d_aerial_amd.mesh --clean --decimate R writes."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_scene as MS
import test_mesh_clean as C
import test_mesh_decimate as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _dev(v, f):
    return torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(f, np.int32)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same_mesh(V, F, v, f):
    assert tuple(V.shape) == v.shape and tuple(F.shape) == f.shape
    assert np.array_equal(_bits(V.cpu().numpy()), _bits(v)) and np.array_equal(F.cpu().numpy(), f)


def _gpu_adjacency(n, f):
    from deep3d_aerial_amd import mesh

    offset, nbr, fixed = mesh.adjacency(torch.from_numpy(np.ascontiguousarray(f, np.int32)).cuda(), n)
    return offset.cpu().numpy(), nbr[:int(offset[-1])].cpu().numpy(), fixed.cpu().numpy()


_NUMPY = {}


def _numpy(fn, v, f, *args, **kw):
    """fn(v, f, ...) of the restatement, computed once per process for the same arrays and settings and never changed (the
    rounds of a run repeat between the settings of a case, and tests/test_uninitialised_gpu.py runs a case three times)."""
    v, f = np.ascontiguousarray(v), np.ascontiguousarray(f)
    key = (fn.__name__, v.dtype.str, v.shape, v.tobytes(), f.dtype.str, f.shape, f.tobytes(), args, tuple(sorted(kw.items())))
    if key not in _NUMPY:
        _NUMPY[key] = fn(v, f, *args, **kw)
    return _NUMPY[key]


def _check_round(v, f, goal):
    """One round of the kernels against the restatement, pass by pass; returns the restatement's round."""
    from deep3d_aerial_amd import mesh

    V, F = _dev(v, f)
    d = {}
    V2, F2, won = mesh.decimate_round(V, F, goal, detail=d)
    w = _numpy(T.decimate_round_numpy, v, f, goal)
    g = lambda k: d[k].cpu().numpy()
    assert np.array_equal(g("face_offset"), w["face_offset"]) and np.array_equal(g("face_index"), w["face_index"])
    assert np.array_equal(g("quadric").view(np.int64), w["quadric"].view(np.int64))
    assert np.array_equal(g("offset"), w["offset"]) and np.array_equal(g("nbr"), w["nbr"]) and np.array_equal(g("fixed"), w["fixed"])
    assert np.array_equal(g("edges"), w["edges"])
    assert np.array_equal(_bits(g("target")), _bits(w["target"])) and np.array_equal(_bits(g("cost")), _bits(w["cost"]))
    assert np.array_equal(g("key"), w["key"])                       # validity is key >= 0
    assert int(d["threshold"][0]) == w["threshold"] and d["eligible"] == w["eligible"]
    assert np.array_equal(g("claim"), w["claim"])
    assert np.array_equal(g("win"), w["win"]) and won == w["winners"]
    _same_mesh(V2, F2, w["vertices"], w["faces"])
    if won == 0:
        assert V2 is V and F2 is F
    return w


def _check_run(v, f, **kw):
    """Every round in lockstep, then mesh.decimate as a whole and a second run; returns (vertices, faces, info)."""
    from deep3d_aerial_amd import mesh

    wv, wf, winfo = _numpy(T.decimate_numpy, v, f, **kw)
    goal = winfo["target_faces"]
    cv, cf = np.asarray(v, np.float32), np.asarray(f, np.int32)
    for _ in range(winfo["rounds"]):
        w = _check_round(cv, cf, goal)
        cv, cf = w["vertices"], w["faces"]
    V, F = _dev(v, f)
    info = {}
    V2, F2 = mesh.decimate(V, F, info=info, **kw)
    _same_mesh(V2, F2, wv, wf)
    assert {k: info[k] for k in winfo} == winfo
    V3, F3 = mesh.decimate(V, F, **kw)
    assert torch.equal(V3.view(torch.int32), V2.view(torch.int32)) and torch.equal(F3, F2)   # the same bits on a second run
    return wv, wf, winfo


CASES = {"grid": lambda: T.grid_mesh(24), "noisy_grid": lambda: T.grid_mesh(24, 0.02, 3), "sphere": T.sphere_mesh, "cone": lambda: T.cone_mesh(1500),
         "two_free": T.two_free_mesh, "tetrahedron": lambda: C.HAND["tetrahedron"], "fan": lambda: C.HAND["fan"]}


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_pass_and_whole_runs_are_bit_equal_to_numpy(name):
    v, f = CASES[name]()
    if name == "cone":
        assert np.bincount(f.ravel()).max() == 1500
    # every neighbourhood around the cone's apex holds the apex, so a round collapses one edge there: a few rounds are enough
    cap = {"max_rounds": 4} if name == "cone" else {}
    for kw in ({"ratio": 0.5}, {"ratio": 0.25}, {"target_faces": max(len(f) // 10, 1)}):
        wv, wf, info = _check_run(v, f, **kw, **cap)
        if name in ("grid", "noisy_grid", "sphere", "cone"):
            T.check_properties(v, f, wv, wf, adjacency=_gpu_adjacency)
            assert info["stalled"] or (info["hit_max_rounds"] if cap else len(wf) in (info["target_faces"], info["target_faces"] - 1))
        print(name, kw, info["rounds"], info["faces_out"], info["stalled"])


def test_planar_grid_tetrahedron_and_adjacent_edges():
    from deep3d_aerial_amd import mesh

    v, f = T.grid_mesh(24)
    info = {}
    V, F = mesh.decimate(*_dev(v, f), ratio=0.25, info=info)
    V, F = V.cpu().numpy(), F.cpu().numpy()
    assert not info["stalled"] and not info["hit_max_rounds"] and len(F) in (264, 265) and info["faces_out"] == len(F)
    assert (V[:, 2].view(np.int32) == 0).all() and abs(T._areas(V, F).sum() - 529.0) < 1e-9
    T.check_properties(v, f, V, F, adjacency=_gpu_adjacency)
    v, f = C.HAND["tetrahedron"]
    Vd, Fd = _dev(v, f)
    info = {}
    V, F = mesh.decimate(Vd, Fd, ratio=0.5, info=info)
    assert info["stalled"] and info["rounds"] == 1 and info["collapses"] == [0] and V is Vd and F is Fd
    v, f = T.two_free_mesh()
    d = {}
    _, F2, won = mesh.decimate_round(*_dev(v, f), len(f) - 4, detail=d)
    key, win = d["key"].cpu().numpy(), d["win"].cpu().numpy()
    el = np.nonzero((key >= 0) & (key <= int(d["threshold"][0])))[0]
    assert len(el) == 2 and won == 1 and win[el[np.argmin(key[el])]] == 1 and win.sum() == 1 and F2.shape[0] == len(f) - 2


def test_off_returns_the_input_tensors_and_errors():
    from deep3d_aerial_amd import mesh

    V, F = _dev(*T.grid_mesh(8))
    for kw in ({}, {"ratio": 1.0}, {"target_faces": int(F.shape[0])}, {"target_faces": 10 ** 6}):
        info = {}
        V2, F2 = mesh.decimate(V, F, info=info, **kw)
        assert V2 is V and F2 is F and info["rounds"] == 0 and info["faces_out"] == F.shape[0]
    info = {}
    V2, F2 = mesh.decimate(V, F, ratio=0.3, max_rounds=2, info=info)
    assert info["hit_max_rounds"] and info["rounds"] == 2 and F2.shape[0] > info["target_faces"]
    with pytest.raises(ValueError, match="outside"):
        mesh.decimate(V, F + 100, ratio=0.5)
    bad = F.clone()
    bad[3, 1] = bad[3, 0]
    with pytest.raises(ValueError, match="repeated index"):
        mesh.decimate(V, bad, ratio=0.5)
    E = torch.zeros((0, 3), dtype=torch.int32, device="cuda")
    V3, F3 = mesh.decimate(V, E, ratio=0.5)
    assert V3 is V and F3 is E


def _raw_mesh(views, border, voxel):
    from deep3d_aerial_amd import mesh

    mv = [mesh.MeshView(x["K"], x["E"], torch.from_numpy(x["depth"]).cuda(), torch.from_numpy(x["confidence"]).cuda()) for x in views]
    return mesh.depth_to_mesh(mv, mesh.MeshGrid(border, voxel))


@pytest.mark.parametrize("name", ["boxes", "sphere"])
def test_scene_meshes_are_bit_equal_to_numpy(name):
    from deep3d_aerial_amd import mesh

    border, voxel, views, _ = MS.SCENES[name]()
    V, F = mesh.clean(*_raw_mesh(views, border, voxel), min_faces=20, smooth=1)
    v, f = V.cpu().numpy(), F.cpu().numpy()
    assert len(f) > 2000
    wv, wf, info = _check_run(v, f, ratio=0.3)
    T.check_properties(v, f, wv, wf, adjacency=_gpu_adjacency)
    assert info["stalled"] or len(wf) in (info["target_faces"], info["target_faces"] - 1)
    print(name, len(f), info["rounds"], info["faces_out"], info["stalled"])


@pytest.mark.parametrize("seed,n,m,hub", [(0, 50, 200, 0), (1, 3000, 2000, 0), (2, 20000, 30000, 1500)])
def test_random_soups_do_not_fault_and_are_bit_equal_to_numpy(seed, n, m, hub):
    """Non-manifold input, no quality claim.  The soup's faces with a repeated index are what decimate refuses, so they are taken
    out first; duplicated faces, both windings and the hub vertex stay."""
    import test_mesh_clean_gpu as CG
    from deep3d_aerial_amd import mesh

    v, f = CG._soup(seed, n, m, hub)
    with pytest.raises(ValueError, match="repeated index"):
        mesh.decimate(*_dev(v, f), ratio=0.5)
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])]
    if hub:
        assert (np.bincount(f.ravel(), minlength=n) > 1000).any()
    _check_run(v, f, ratio=0.8, max_rounds=6)


def test_decimation_beats_a_coarser_voxel_at_equal_face_count():
    """Today's only way to a mesh of T faces is a coarser voxel.  boxes_scene(holes=False) at voxel s (smoothed once) decimated to the
    face count of the mesh at voxel 2 s; all three rasterised on one grid of cell s: the decimated mesh has no more faces than the
    coarse one and its RMS height difference from the fine mesh's DSM is smaller than the coarse mesh's.  No margin."""
    from deep3d_aerial_amd import dsm, mesh

    border, s, views, _ = MS.boxes_scene(holes=False)
    Vf, Ff = mesh.clean(*_raw_mesh(views, border, s), smooth=1)
    Vc, Fc = _raw_mesh(views, border, 2 * s)
    info = {}
    Vd, Fd = mesh.decimate(Vf, Ff, target_faces=int(Fc.shape[0]), info=info)
    grid = dsm.DsmGrid(border[:4], s)
    hf, hc, hd = (dsm.mesh_to_dsm(V, F, grid).cpu().numpy().astype(np.float64) for V, F in ((Vf, Ff), (Vc, Fc), (Vd, Fd)))
    ok = np.isfinite(hf) & np.isfinite(hc) & np.isfinite(hd)
    rms = lambda h: float(np.sqrt(np.mean((h[ok] - hf[ok]) ** 2)))
    print("fine %d faces, coarse %d faces (rms %.5f), decimated %d faces (rms %.5f), rounds %d, stalled %s, cells %d" % (
        Ff.shape[0], Fc.shape[0], rms(hc), Fd.shape[0], rms(hd), info["rounds"], info["stalled"], int(ok.sum())))
    assert ok.sum() > 1000
    assert Fd.shape[0] <= Fc.shape[0]
    assert rms(hd) < rms(hc)


# ----------------------------------------------------------------------------------------
# the pipeline stage and the files
# ----------------------------------------------------------------------------------------
RATIO = 0.4


def _scene_setup():
    import ortho_scene as OS
    import texture_scene as TS

    scene = OS.ImageSceneViews()
    border, voxel = TS.scene_border(scene)
    return scene, border, voxel


def _cli_decimated(tmp_path, scene, border, voxel):
    """python -m deep3d_aerial_amd.mesh --clean RAW.ply --smooth 1 --decimate R on the undecimated mesh: the file's bytes."""
    from deep3d_aerial_amd import mesh

    views = []
    for i in range(len(scene)):
        it = scene[i]
        views.append(mesh.MeshView(it["outcam"][1, :3, :3], it["outcam"][0], torch.from_numpy(scene.views[i]["depth"]).cuda(),
                                   torch.from_numpy(scene.views[i]["confidence"]).cuda()))
    V, F = mesh.depth_to_mesh(views, mesh.MeshGrid(border, voxel))
    raw = str(tmp_path / "raw.ply")
    mesh.write_ply(raw, V, F)
    out = tmp_path / "cli.ply"
    res = subprocess.run([sys.executable, "-m", "deep3d_aerial_amd.mesh", "--clean", raw, "--out", str(out), "--smooth", "1", "--decimate",
                          repr(RATIO)], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")),
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    return out.read_bytes(), V.cpu().numpy(), F.cpu().numpy()


def test_predict_and_fuse_writes_the_decimated_mesh_the_cli_writes_and_textures_it(tmp_path):
    import mesh_decimate_scene as DS
    from deep3d_aerial_amd import mesh, texture

    scene, border, voxel = _scene_setup()
    DS.run(str(tmp_path / "a"), border, voxel, RATIO)
    cli, v, f = _cli_decimated(tmp_path, scene, border, voxel)
    assert cli == (tmp_path / "a" / "mesh.ply").read_bytes()
    Vd, Fd = mesh.read_ply(str(tmp_path / "a" / "mesh.ply"))
    sv = C.smooth_numpy(v, f, 1)
    wv, wf, info = T.decimate_numpy(sv, f, ratio=RATIO)
    assert np.array_equal(_bits(Vd), _bits(wv)) and np.array_equal(Fd, wf) and 100 < len(Fd) < len(f)
    assert info["stalled"] or len(Fd) in (info["target_faces"], info["target_faces"] - 1)
    tex = texture.read_textured_ply(str(tmp_path / "a" / "tex.ply"))
    assert len(tex[1]) == len(Fd) and np.array_equal(tex[1], Fd)   # the texture is laid on the decimated mesh


def _launch(n_ranks, out_dir, border, voxel):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "mesh_decimate_scene.py"), str(out_dir), ",".join(repr(b) for b in border),
           repr(voxel), repr(RATIO)]
    res = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-3000:])
    return res.stdout


def test_two_ranks_write_the_decimated_mesh_one_rank_and_the_cli_write(tmp_path):
    from deep3d_aerial_amd import mesh, texture

    scene, border, voxel = _scene_setup()
    out1 = _launch(1, tmp_path / "one", border, voxel)
    out2 = _launch(2, tmp_path / "two", border, voxel)
    assert "rank 0/1" in out1 and "rank 0/2" in out2 and "rank 1/2" in out2
    one = (tmp_path / "one" / "mesh.ply").read_bytes()
    assert one == (tmp_path / "two" / "mesh.ply").read_bytes()
    assert one == _cli_decimated(tmp_path, scene, border, voxel)[0]
    assert (tmp_path / "one" / "tex.ply").read_bytes() == (tmp_path / "two" / "tex.ply").read_bytes()
    Fd = mesh.read_ply(str(tmp_path / "two" / "mesh.ply"))[1]
    assert np.array_equal(texture.read_textured_ply(str(tmp_path / "two" / "tex.ply"))[1], Fd)
