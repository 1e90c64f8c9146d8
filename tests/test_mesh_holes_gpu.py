"""The hole-closing kernels (csrc/mesh_holes.hip) on the GPU: every output of mesh.boundary_loops, the loop sums s (fp64), the
qualify flags and the vertices and faces of mesh.close_holes bit-equal to the numpy restatement of tests/test_mesh_holes.py, on
its hand cases, on the numpy meshes of the scenes of tests/mesh_scene.py, on a grid with 4096 holes and on a loop of 1024 edges;
the step off; what closing does to the mesh DSM and to decimation's fixed vertices; the PLY of predict_and_fuse(mesh={...,
"close_holes": N}) equal to the one python -m deep3d_aerial_amd.mesh --mvs ... --close_holes N writes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_scene as MS
import test_mesh_holes as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
LOOP_KEYS = ("boundary", "out", "in", "successor", "owner", "label", "count", "bad")
PLAN_KEYS = ("qualify", "position", "vertex_offset", "face_offset")


def _dev(v, f):
    return torch.from_numpy(np.array(v, np.float32)).cuda(), torch.from_numpy(np.array(f, np.int32)).cuda()   # copies: a scene's arrays are read-only


def _check(v, f, max_edges):
    """Every pass and the whole step against the restatement; returns (the restatement's detail, info)."""
    from deep3d_aerial_amd import mesh

    V, F = _dev(v, f)
    wv, wf, w = T.close_holes_numpy(v, f, max_edges)
    loops = mesh.boundary_loops(F, len(v))
    for k in LOOP_KEYS:
        assert np.array_equal(loops[k].cpu().numpy(), w[k]), k
    assert loops["rounds"] >= 1
    p = mesh.plan_holes(V, F, max_edges, loops=loops)
    assert np.array_equal(p["s"].cpu().numpy().view(np.int64), w["s"].view(np.int64))
    assert np.array_equal(T._bits(p["centroid"].cpu().numpy()), T._bits(w["centroid"]))
    for k in PLAN_KEYS:
        assert np.array_equal(p[k].cpu().numpy(), w[k]), k
    assert (p["holes"], p["faces_added"]) == (w["holes"], w["faces_added"])
    info = {}
    V2, F2 = mesh.close_holes(V, F, max_edges, info=info)
    assert tuple(V2.shape) == wv.shape and tuple(F2.shape) == wf.shape
    assert np.array_equal(T._bits(V2.cpu().numpy()), T._bits(wv)) and np.array_equal(F2.cpu().numpy(), wf)
    # rounds is no function of the mesh: a hooking launch may or may not see a parent another workgroup has just lowered
    assert {k: info[k] for k in w["info"]} == w["info"] and info["rounds"] >= 1
    if w["holes"] == 0:
        assert V2 is V and F2 is F
    else:
        V3, F3 = mesh.close_holes(V2, F2, max_edges)       # a second call closes nothing
        assert V3 is V2 and F3 is F2
    return w, info


@pytest.mark.parametrize("name", sorted(T.HAND) + sorted(T.SCENES))
def test_every_pass_and_the_closed_mesh_are_bit_equal_to_numpy(name):
    v, f = T.case(name)
    for max_edges in (30, 100):
        w, info = _check(v, f, max_edges)
        print(name, max_edges, info)
    if name in T.SCENES:
        assert info["holes_closed"] > 0


def test_many_loops_are_numbered_by_scans_past_one_tile():
    """A 256 x 256 grid without the fan of every fourth interior vertex in both directions: 64 x 64 six-edge holes, more than
    one scan tile of 4096 values among 66049 vertices."""
    v, f = T.grid_mesh(256)
    centres = [i + j * 257 for j in range(2, 255, 4) for i in range(2, 255, 4)]
    f = T.without_fans(f, centres)
    w, info = _check(v, f, 30)
    assert info["holes_closed"] == len(centres) == 4096 and info["faces_added"] == 6 * 4096
    assert info["loops"] == 4097 and info["skipped_large"] == 1      # the grid's border


def test_a_loop_of_1024_edges_closes_and_1023_is_too_few():
    from deep3d_aerial_amd import mesh

    v, f = T.annulus(mesh.HOLE_MAX_EDGES)
    w, info = _check(v, f, mesh.HOLE_MAX_EDGES)
    assert info["holes_closed"] == 1 and info["faces_added"] == 1024 and info["skipped_outer"] == 1
    w, info = _check(v, f, mesh.HOLE_MAX_EDGES - 1)
    assert info["holes_closed"] == 0 and info["skipped_large"] == 2


def test_a_face_with_a_repeated_index_is_refused_only_when_the_step_is_on():
    from deep3d_aerial_amd import mesh

    V, F = _dev(*T.HAND["hexagon_annulus"])
    bad = F.clone()
    bad[3, 1] = bad[3, 0]
    with pytest.raises(ValueError, match="repeated index"):
        mesh.close_holes(V, bad, 30)
    with pytest.raises(ValueError, match="repeated index"):
        mesh.clean(V, bad, close_holes=30)
    with pytest.raises(ValueError, match="repeated index"):
        mesh.boundary_loops(bad, V.shape[0])
    V2, F2 = mesh.clean(V, bad)
    assert V2 is V and F2 is bad
    V2, F2 = mesh.close_holes(V, bad, 0)
    assert V2 is V and F2 is bad
    with pytest.raises(ValueError, match="outside"):
        mesh.close_holes(V, F + 100, 30)


def test_the_step_off_returns_what_clean_returns_today():
    import test_mesh_clean as C
    from deep3d_aerial_amd import mesh

    V, F = _dev(*T.HAND["hexagon_annulus"])
    for kw in ({}, {"close_holes": 0}):
        V2, F2 = mesh.clean(V, F, **kw)
        assert V2 is V and F2 is F
    info = {}
    V2, F2 = mesh.close_holes(V, F, 0, info=info)
    assert V2 is V and F2 is F and info["holes_closed"] == 0
    E = torch.zeros((0, 3), dtype=torch.int32, device="cuda")
    V2, F2 = mesh.close_holes(V, E, 30)
    assert V2 is V and F2 is E
    v, f = T.scene("boxes")
    Vs, Fs = _dev(v, f)
    a = mesh.clean(Vs, Fs, min_faces=20, smooth=1)
    b = mesh.clean(Vs, Fs, min_faces=20, smooth=1, close_holes=0)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    cv, cf = C.clean_numpy(v, f, 20, 0.0, 1)
    assert np.array_equal(T._bits(a[0].cpu().numpy()), T._bits(cv)) and np.array_equal(a[1].cpu().numpy(), cf)
    # on: removal, hole closing, smoothing, in that order
    info = {}
    Vc, Fc = mesh.clean(Vs, Fs, min_faces=20, smooth=1, close_holes=30, info=info)
    rv, rf = C.remove_numpy(v, f, 20)
    hv, hf, w = T.close_holes_numpy(rv, rf, 30)
    sv = C.smooth_numpy(hv, hf, 1)
    assert w["holes"] > 0 and info["close_holes"]["holes_closed"] == w["holes"] and "faces_removed" in info
    assert np.array_equal(T._bits(Vc.cpu().numpy()), T._bits(sv)) and np.array_equal(Fc.cpu().numpy(), hf)


def test_closing_fills_the_mesh_dsm_with_the_plane_and_changes_no_valid_cell():
    from deep3d_aerial_amd import dsm, mesh

    c = 2.5
    v, f = T.grid_mesh(12, 12, c)
    f = T.without_fans(f, [6 + 6 * 13])
    V, F = _dev(v, f)
    unit = 0.25
    grid = dsm.DsmGrid([0.0, 12.0, 0.0, 12.0], unit)
    before = dsm.mesh_to_dsm(V, F, grid).cpu().numpy()
    V2, F2 = mesh.close_holes(V, F, 30)
    assert V2.shape[0] == V.shape[0] + 1 and F2.shape[0] == F.shape[0] + 6
    after = dsm.mesh_to_dsm(V2, F2, grid).cpu().numpy()
    i, j = np.mgrid[0:grid.height, 0:grid.width]
    x = grid.x_min + (j + 0.5) * unit
    y = grid.y_max - (i + 0.5) * unit
    inside = (x > 5) & (x < 7) & (y > 5) & (y < 7) & (x - y > -1) & (x - y < 1)     # strictly inside the hexagon around (6, 6)
    assert inside.sum() > 20 and np.isnan(before[inside]).all()
    assert (after[inside].view(np.int32) == np.float32(c).view(np.int32)).all()
    valid = ~np.isnan(before)
    assert valid.sum() > 2000 and np.array_equal(after[valid].view(np.int32), before[valid].view(np.int32))


def test_closing_frees_exactly_the_vertices_on_the_closed_loops_for_decimation():
    from deep3d_aerial_amd import mesh

    border, s, views, _ = MS.boxes_scene(holes=False)
    mv = [mesh.MeshView(x["K"], x["E"], torch.from_numpy(x["depth"]).cuda(), torch.from_numpy(x["confidence"]).cuda()) for x in views]
    V, F = mesh.clean(*mesh.depth_to_mesh(mv, mesh.MeshGrid(border, s)), smooth=1)
    fixed = int(mesh.adjacency(F, V.shape[0])[2].sum())
    info = {}
    V2, F2 = mesh.close_holes(V, F, 30, info=info)
    fixed2 = int(mesh.adjacency(F2, V2.shape[0])[2].sum())
    print("fixed %d -> %d, %s" % (fixed, fixed2, info))
    assert info["holes_closed"] > 0 and info["faces_added"] >= 3 * info["holes_closed"]
    assert fixed - fixed2 == info["faces_added"]                     # a closed loop of k edges has k vertices


def test_predict_and_fuse_writes_the_closed_mesh_the_cli_writes(tmp_path):
    import pipeline_scene as PS
    import test_mesh_gpu as G
    from deep3d_aerial_amd import mesh, pipeline

    border, voxel = G._border(tmp_path)
    scene = PS.SceneViews()
    settings = MS.pipeline_settings(str(tmp_path / "a" / "mesh.ply"), border, voxel)
    settings.update(close_holes=30)
    mvs = tmp_path / "a" / "MVS"
    pipeline.predict_and_fuse(PS.SceneModel(scene), scene, str(mvs), checker=PS.checker(), fusion_num=PS.FUSION_NUM,
                              min_geo_consist_num=3, filter_sources=False, mesh=settings)
    out = tmp_path / "cli.ply"
    res = subprocess.run([sys.executable, "-m", "deep3d_aerial_amd.mesh", "--mvs", str(mvs), "--out", str(out),
                          "--border=%s" % ",".join(repr(b) for b in border), "--voxel=%r" % voxel, "--close_holes", "30"], cwd=ROOT,
                         env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")),
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    assert out.read_bytes() == (tmp_path / "a" / "mesh.ply").read_bytes()
    views = []
    for i in range(len(scene)):
        it = scene[i]
        views.append(mesh.MeshView(it["outcam"][1, :3, :3], it["outcam"][0], torch.from_numpy(scene.views[i]["depth"]).cuda(),
                                   torch.from_numpy(scene.views[i]["confidence"]).cuda()))
    V, F = mesh.depth_to_mesh(views, mesh.MeshGrid(border, voxel))
    wv, wf, w = T.close_holes_numpy(V.cpu().numpy(), F.cpu().numpy(), 30)
    Vc, Fc = mesh.read_ply(str(out))
    assert np.array_equal(T._bits(Vc), T._bits(wv)) and np.array_equal(Fc, wf) and len(Fc) > 100
    print("pipeline mesh:", w["info"])
