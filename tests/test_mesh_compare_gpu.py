"""The comparison of a surface mesh with a reference cloud on the GPU (csrc/mesh_sample.hip, mesh_compare.sample / face_error /
compare): offsets, xyz and face bit-equal to the numpy restatement of tests/mesh_compare_scene.py -- on one face of many sizes, past
one and two scan tiles, on tiles that end on a face boundary, on runs of faces without samples, on empty meshes, on one large face
among thousands of small ones --; the refusals of sample() before anything is emitted; the face error against np.add.at and
np.maximum.at; compare() against the restatements of the search (tests/test_cloud_compare.py: the cell list on the whole scene, the
brute force over all pairs on a part of either direction) on the restated samples, in any face and reference order; the
two-triangle square that the vertices alone get wrong; and the file tool."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_compare_scene as MS
import test_cloud_compare as TCC
import test_mesh_compare as TMC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _dev(v, f):
    return torch.from_numpy(np.ascontiguousarray(v, np.float32).reshape(-1, 3)).cuda(), torch.from_numpy(np.ascontiguousarray(f, np.int32).reshape(-1, 3)).cuda()


def _check(v, f, s):
    """The GPU's samples of the mesh against the restatement, bit for bit; -> the restatement."""
    from deep3d_aerial_amd import mesh_compare as MC

    want = MS.sample_numpy(v, f, s)
    xyz, face, offsets = MC.sample(*_dev(v, f), s)
    assert xyz.is_cuda and xyz.dtype == torch.float32 and face.dtype == torch.int32 and offsets.dtype == torch.int32
    assert tuple(offsets.shape) == (len(f) + 1,) and tuple(xyz.shape) == (len(want[0]), 3) and tuple(face.shape) == (len(want[0]),)
    assert np.array_equal(offsets.cpu().numpy(), want[2])
    assert np.array_equal(face.cpu().numpy(), want[1])
    assert np.array_equal(MS.bits(xyz.cpu().numpy()), MS.bits(want[0]))
    return want


# ----------------------------------------------------------------------------------------
# the samples
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TMC.hand_cases(), ids=lambda c: c[0])
def test_the_hand_cases(case):
    _, v, f, s, n, want = case
    got = _check(v, f, s)
    assert np.diff(got[2]).tolist() == [k * k for k in n]
    if want is not None:
        assert np.array_equal(MS.bits(got[0]), MS.bits(np.float32(want).reshape(-1, 3)))


@pytest.mark.parametrize("n", [1, 2, 3, 5, 17, 300])
def test_one_face(n):
    v, f, s = MS.one_face(n, seed=n)
    assert len(_check(v, f, s)[0]) == n * n   # n = 300: 352 tiles inside one face, and the rows around every square up to 299^2


@pytest.mark.parametrize("k", [4097, 2 * 4096 + 1])
def test_unit_faces_past_one_and_two_scan_tiles(k):
    v, f = MS.unit_faces(k, seed=k)
    assert len(_check(v, f, 1.0)[0]) == k


@pytest.mark.parametrize("shift", [0, 1, 37])
def test_a_tile_that_ends_on_a_face_boundary(shift):
    # 256 - shift unit faces, then one face of 1600 samples, then unit faces again: with shift = 0 the first tile ends exactly where
    # the large face begins, and 256 + 1600 = 7 * 256 + 64 samples later a tile begins inside it and ends in the unit faces
    v, f = MS.join([MS.unit_faces(256 - shift, seed=1), MS.big_face(40, 200.0), MS.unit_faces(300, seed=2, origin=400.0)])
    w = _check(v, f, 1.0)
    assert w[2][256 - shift] == 256 - shift and w[2][257 - shift] == 256 - shift + 1600


@pytest.mark.parametrize("run", [1, 255, 256, 700])
def test_runs_of_faces_without_samples_before_between_and_after_sampled_faces(run):
    gone = lambda seed: MS.empty_faces(run, seed)
    v, f = MS.join([gone(1), MS.unit_faces(3, seed=1), gone(2), MS.big_face(5, 200.0), gone(3), MS.unit_faces(130, seed=2, origin=300.0), gone(4),
                    gone(5), MS.unit_faces(1, seed=3, origin=500.0), gone(6)])
    w = _check(v, f, 1.0)
    assert len(w[0]) == 3 + 25 + 130 + 1 and len(f) == 6 * run + 135
    _check(v, f[::-1].copy(), 1.0)


def test_no_face_and_only_faces_without_samples():
    from deep3d_aerial_amd import mesh_compare as MC

    v, f = MS.unit_faces(4)
    for vv, ff in ((v, f[:0]), (v[:0], f[:0]), MS.empty_faces(1), MS.empty_faces(700)):
        w = _check(vv, ff, 1.0)
        assert len(w[0]) == 0 and not w[2].any()
    # and the face error and a whole comparison of such a mesh
    vv, ff = MS.empty_faces(9)
    total, keyed, worst = MC.face_error(torch.zeros(0, dtype=torch.int32).cuda(), torch.zeros(0, dtype=torch.int32).cuda(), 9)
    assert total.tolist() == [0] * 9 and keyed.tolist() == [0] * 9 and worst.tolist() == [-1] * 9
    assert all(tuple(t.shape) == (0,) for t in MC.face_error(torch.zeros(0, dtype=torch.int32).cuda(), torch.zeros(0, dtype=torch.int32).cuda(), 0))
    ref = torch.rand(50, 3).cuda()
    result, found = MC.compare(*_dev(vv, ff), ref, [0.0, 1.0, 0.0, 1.0, 0.0, 1.0], 0.25, [0.1], 0.5)
    assert result["mesh"] == {"faces": 9, "sampled_faces": 0, "samples": 0, "spacing": 0.5}
    assert result["cloud"]["points"] == 0 and result["reference"]["beyond"] == 50 and result["thresholds"][0]["fscore"] == 0.0
    assert found["faces"][2].tolist() == [-1] * 9


def test_one_large_face_among_5000_small_ones_in_shuffled_order():
    v, f = MS.join([MS.unit_faces(5000, seed=4), MS.big_face(100, 200.0)])
    f = f[np.random.default_rng(5).permutation(len(f))]
    w = _check(v, f, 1.0)
    assert len(w[0]) == 5000 + 10000


def test_dtypes_and_shapes_are_refused():
    from deep3d_aerial_amd import mesh_compare as MC

    v, f = _dev(*MS.unit_faces(4))
    for bad_v, bad_f, msg in ((v.double(), f, "vertices"), (v[:, :2], f, "vertices"), (v, f.long(), "faces"), (v, f[:, :2], "faces"),
                              (v, f + 10, "outside"), (v, f - 1, "outside")):
        with pytest.raises(ValueError, match=msg):
            MC.sample(bad_v, bad_f, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MC.sample(v, f.cpu(), 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MC.compare(v, f, torch.zeros(5, 3), [0.0, 4.0, 0.0, 4.0, 0.0, 4.0], 1.0, [0.5], 0.5)


def _peak_of(call):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with pytest.raises(ValueError) as err:
        call()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, str(err.value)


def test_sample_refuses_a_clipped_face_and_too_many_samples_before_it_emits():
    from deep3d_aerial_amd import mesh_compare as MC

    # one face 4000 long at a spacing of 0.1: 40000 spacings > 32768.  Only the count runs: xyz alone would be 12 * 2^30 bytes.
    v, f = _dev(np.float32([[0, 0, 0], [4000, 0, 0], [0, 3000, 0]]), np.int32([[0, 1, 2]]))
    peak, text = _peak_of(lambda: MC.sample(v, f, 0.1))
    assert peak < 1 << 20 and "0.1" in text and "1 of 1 faces" in text and "32768" in text
    # 2000 faces of 10^2 samples with max_samples one short: 3.2 MB of samples are not allocated
    v, f = _dev(*MS.join([MS.big_face(10, 30.0 * k) for k in range(2000)]))
    peak, text = _peak_of(lambda: MC.sample(v, f, 1.0, max_samples=199999))
    assert peak < 1 << 20 and "200000" in text and "199999" in text and "1.0" in text and "2000 faces" in text
    xyz, face, offsets = MC.sample(v, f, 1.0, max_samples=200000)
    assert tuple(xyz.shape) == (200000, 3) and int(offsets[-1]) == 200000
    # more than 2^31 - 1 samples without a clipped face: three faces of 30000^2
    v, f = _dev(*MS.join([MS.big_face(30000, 0.0)] * 3))
    peak, text = _peak_of(lambda: MC.sample(v, f, 1.0))
    assert peak < 1 << 20 and "2700000000" in text


# ----------------------------------------------------------------------------------------
# the face error
# ----------------------------------------------------------------------------------------
def test_the_face_error_is_the_scatter_restatement():
    from deep3d_aerial_amd import mesh_compare as MC

    rng = np.random.default_rng(6)
    # faces with no sample (2, 5, the last three), faces whose samples are all unkeyed (1, 7), one face of 90 000 samples (4), runs that
    # straddle waves and tiles, single samples
    counts = [3, 70, 0, 1, 90000, 0, 257, 130, 1, 1, 64, 63, 65, 1000, 0, 0, 0]
    face = np.repeat(np.arange(len(counts)), counts).astype(np.int32)
    e = rng.integers(0, 1025, len(face)).astype(np.int32)
    e[rng.random(len(face)) < 0.1] = -1
    e[(face == 1) | (face == 7)] = -1
    want = MS.face_error_numpy(e, face, len(counts))
    assert want[1][[1, 2, 7]].tolist() == [0, 0, 0] and want[2][[1, 2, 7]].tolist() == [-1, -1, -1] and want[1][4] > 80000
    for ee, ff in ((e, face), (e[5:], face[5:]), (e[::-1].copy(), face[::-1].copy())):
        w = MS.face_error_numpy(ee, ff, len(counts))
        got = MC.face_error(torch.from_numpy(ee).cuda(), torch.from_numpy(ff).cuda(), len(counts))
        assert got[0].dtype == torch.int64 and got[1].dtype == torch.int32 and got[2].dtype == torch.int32
        assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(got, w))
    # the samples of a face need not be consecutive for the result to hold, and a large e sums in 64 bits
    p = rng.permutation(len(face))
    big = np.where(e >= 0, e + (1 << 30), e).astype(np.int32)
    got = MC.face_error(torch.from_numpy(big[p]).cuda(), torch.from_numpy(face[p]).cuda(), len(counts))
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(got, MS.face_error_numpy(big[p], face[p], len(counts))))


def test_the_face_error_on_short_runs_of_three_faces_that_come_back():
    """200 samples over 3 faces as a, a, b, a, b, b, a, ...: runs of one and two, each face again and again within a wave, some
    samples unkeyed.  Equal faces that are not adjacent are separate runs; the sums must not join them twice or lose one."""
    from deep3d_aerial_amd import mesh_compare as MC

    rng = np.random.default_rng(7)
    face = np.resize(np.array([0, 0, 1, 0, 1, 1, 0, 2, 1, 2, 2, 0, 2], np.int32), 200)
    e = rng.integers(0, 1025, 200).astype(np.int32)
    e[rng.random(200) < 0.2] = -1
    assert (np.diff(face) != 0).sum() > 120 and 20 < (e < 0).sum() < 70
    want = MS.face_error_numpy(e, face, 3)
    assert (want[1] > 30).all()
    got = MC.face_error(torch.from_numpy(e).cuda(), torch.from_numpy(face).cuda(), 3)
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(got, want))


# ----------------------------------------------------------------------------------------
# the comparison
# ----------------------------------------------------------------------------------------
_SCENE = {}


def scene():
    """The height field, its restated samples and the restated search in both directions, computed once."""
    if not _SCENE:
        from deep3d_aerial_amd import cloud

        v, f, ref, border, h, s = MS.height_field()
        g = cloud.CloudGrid(border, h)
        xyz, face, offsets = MS.sample_numpy(v, f, s)
        _SCENE.update(v=v, f=f, ref=ref, border=border, h=h, s=s, grid=g, xyz=xyz, face=face, offsets=offsets,
                      ab=TCC.nearest_cells(xyz, ref, g), ba=TCC.nearest_cells(ref, xyz, g))
    return _SCENE


def test_the_height_field_both_directions_the_statistics_and_the_face_error():
    from deep3d_aerial_amd import cloud_compare as CC, mesh_compare as MC

    sc = scene()
    v, f, ref, xyz, face = sc["v"], sc["f"], sc["ref"], sc["xyz"], sc["face"]
    n = np.diff(sc["offsets"])
    assert 19000 < len(f) < 21000 and len(ref) == 30220 and len(np.unique(n)) >= 4 and (n == 1).any() and n.max() >= 4
    # the cell list of §4.29's test module stands for its brute force over all pairs, which takes minutes on the host for this scene
    # (tests/test_cloud_compare.py holds the two equal); the brute force itself on 2000 samples and on 300 reference points
    rng = np.random.default_rng(0)
    for q, t, got, k in ((xyz, ref, sc["ab"], 2000), (ref, xyz, sc["ba"], 300)):
        part = rng.choice(len(q), k, replace=False)
        brute = TCC.nearest_numpy(q[part], t, sc["grid"])
        assert np.array_equal(brute[0], got[0][part]) and np.array_equal(brute[1], got[1][part])
    taus = [0.05, 0.1, 0.3]
    want = CC.stats(sc["ab"][2], sc["ba"][2], sc["h"], taus, (len(xyz), len(ref)))
    want["mesh"] = {"faces": len(f), "sampled_faces": int((n > 0).sum()), "samples": len(xyz), "spacing": sc["s"]}
    dv, df = _dev(v, f)
    result, found = MC.compare(dv, df, torch.from_numpy(ref).cuda(), sc["border"], sc["h"], taus, sc["s"])
    assert result == want and sorted(found) == ["faces", "reference", "samples"]
    sx, sf, ea, ia = (t.cpu().numpy() for t in found["samples"])
    eb, ib = (t.cpu().numpy() for t in found["reference"])
    assert np.array_equal(MS.bits(sx), MS.bits(xyz)) and np.array_equal(sf, face)
    assert np.array_equal(ea, sc["ab"][0]) and np.array_equal(ia, sc["ab"][1]) and np.array_equal(eb, sc["ba"][0]) and np.array_equal(ib, sc["ba"][1])
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(found["faces"], MS.face_error_numpy(ea, face, len(f))))
    row = result["thresholds"][2]
    assert 0.5 < row["accuracy"] < 1 and 0.5 < row["completeness"] < 1 and result["reference"]["beyond"] > 100
    assert (found["faces"][2] == -1).sum().item() == 0 and (ea == -1).sum() == 0


def test_the_height_field_in_any_face_order_and_any_reference_order():
    from deep3d_aerial_amd import mesh_compare as MC

    sc = scene()
    rng = np.random.default_rng(1)
    pf, pr = rng.permutation(len(sc["f"])), rng.permutation(len(sc["ref"]))
    taus = [0.05, 0.1, 0.3]
    dv, df = _dev(sc["v"], sc["f"])
    first, found = MC.compare(dv, df, torch.from_numpy(sc["ref"]).cuda(), sc["border"], sc["h"], taus, sc["s"])
    dv, df = _dev(sc["v"], sc["f"][pf])
    again, found2 = MC.compare(dv, df, torch.from_numpy(sc["ref"][pr]).cuda(), sc["border"], sc["h"], taus, sc["s"])
    assert again == first
    # e of the reference follows its order; the error of a face follows the face
    assert np.array_equal(found2["reference"][0].cpu().numpy(), found["reference"][0].cpu().numpy()[pr])
    for a, b in zip(found2["faces"], found["faces"]):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()[pf])


def test_two_triangles_are_complete_where_their_four_vertices_are_not():
    """The reason for the feature: a flat square of two triangles against 10 000 reference points on it."""
    from deep3d_aerial_amd import cloud_compare as CC, mesh_compare as MC

    side = 10.0
    v = np.float32([[0, 0, 2], [side, 0, 2], [side, side, 2], [0, side, 2]])
    f = np.int32([[0, 1, 2], [0, 2, 3]])
    rng = np.random.default_rng(3)
    ref = np.concatenate([rng.uniform(0, side, (10000, 2)), np.full((10000, 1), 2.0)], 1).astype(np.float32)
    border, h, tau = [-1.0, 11.0, -1.0, 11.0, 0.0, 4.0], 1.0, 0.02 * side
    # a spacing of tau: every point of the square is within 2 tau / 3 of a sample
    dv, df = _dev(v, f)
    dref = torch.from_numpy(ref).cuda()
    result, found = MC.compare(dv, df, dref, border, h, [tau], tau)
    assert result["thresholds"][0]["completeness"] == 1.0 and result["thresholds"][0]["accuracy"] > 0.99
    assert result["mesh"]["faces"] == 2 and result["mesh"]["sampled_faces"] == 2 and result["mesh"]["samples"] == 2 * 71 * 71
    by_vertices, _ = CC.compare(dv, dref, border, h, [tau])
    assert by_vertices["thresholds"][0]["completeness"] < 0.01


# ----------------------------------------------------------------------------------------
# the file tool
# ----------------------------------------------------------------------------------------
def test_the_file_tool_writes_the_result_and_all_four_files_byte_for_byte(tmp_path):
    from deep3d_aerial_amd import mesh_compare as MC

    v, f, ref, border, h, _ = MS.height_field(seed=2, side=21)
    ref, s = ref[:3000], 1.0
    (tmp_path / "m.ply").write_bytes(MS.ply_mesh_bytes(v, f))
    dt = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("intensity", "<u2")])   # the reference as a LiDAR export in doubles
    rec = np.zeros(len(ref), dt)
    for k, a in enumerate("xyz"):
        rec[a] = ref[:, k]
    (tmp_path / "b.ply").write_bytes(TCC.ply_bytes("binary_little_endian", [("vertex", len(ref), [("double", "x"), ("double", "y"), ("double", "z"),
                                                                                                     ("ushort", "intensity")], rec.tobytes())]))
    out = tmp_path / "cli"
    cmd = [sys.executable, "-m", "deep3d_aerial_amd.mesh_compare", "--mesh", str(tmp_path / "m.ply"), "--reference", str(tmp_path / "b.ply"),
           "--border=%s" % ",".join(repr(x) for x in border), "--max_dist=%r" % h, "--threshold=0.1,0.3", "--spacing=%r" % s,
           "--json", str(out / "r.json"), "--out_samples", str(out / "s.ply"), "--out_accuracy", str(out / "ea.ply"),
           "--out_completeness", str(out / "eb.ply"), "--out_mesh", str(out / "em.ply")]
    r = subprocess.run(["timeout", "-k", "10", "300"] + cmd, cwd=ROOT, capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))
    assert r.returncode == 0, r.stderr[-3000:]
    dv, df = _dev(v, f)
    result, found = MC.compare(dv, df, torch.from_numpy(ref).cuda(), border, h, [0.1, 0.3], s)
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 1 and json.loads(lines[0]) == result == json.loads((out / "r.json").read_text())
    assert 0 < result["thresholds"][0]["fscore"] < result["thresholds"][1]["fscore"] <= 1
    xyz, face, offsets = MS.sample_numpy(v, f, s)
    ea, eb = found["samples"][2].cpu().numpy(), found["reference"][0].cpu().numpy()
    assert (out / "s.ply").read_bytes() == MS.samples_numpy(xyz, face)
    assert (out / "ea.ply").read_bytes() == TCC.error_bytes_numpy(xyz, ea)
    assert (out / "eb.ply").read_bytes() == TCC.error_bytes_numpy(ref, eb)
    total, keyed, _ = MS.face_error_numpy(ea, face, len(f))
    assert (out / "em.ply").read_bytes() == MS.error_mesh_numpy(v, f, total, keyed)
