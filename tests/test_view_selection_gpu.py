"""The view selection on the GPU (csrc/view_select.hip, view_selection.block_references / score / select): bit for bit against
the restatement of tests/view_selection_scene.py -- on the two golden scenes end to end and against the reference's files, on
hand-made models at every boundary of the rule, on the scratch path against the LDS path, in angle mode at the bin edges, on the
block tests' edges, under shuffles of everything whose order must not matter; and the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import view_selection_scene as VS
from deep3d_aerial_amd import sparse_model, view_selection

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _check(model, refs=None, mode="points", angle=view_selection.ANGLE_DEFAULT, lds_images=None):
    """score() of the refs (default: every image) against the restatement, view by view; -> {image id: restated view}."""
    refs = model.image_ids.tolist() if refs is None else list(refs)
    got = view_selection.score(model, refs, mode, angle, lds_images)
    assert got.src.is_cuda and got.seen.dtype == torch.int32 and got.src.dtype == torch.int64 and got.score.dtype == torch.int64
    h = got.host()
    assert h["refs"].tolist() == refs and h["offset"][0] == 0 and len(h["offset"]) == len(refs) + 1 and h["offset"][-1] == len(h["src"])
    want = {}
    for i, r in enumerate(refs):
        v = want[r] = VS.view(model, r, mode, angle)
        a, b = int(h["offset"][i]), int(h["offset"][i + 1])
        assert (int(h["seen"][i]), int(h["max"][i])) == (v["seen"], v["max"]), r
        assert list(zip(h["src"][a:b].tolist(), h["score"][a:b].tolist(), h["count"][a:b].tolist())) == v["sources"], r
    return want


def _ring(n_img, count, first=1):
    """n_img images that all see the same `count` points."""
    return VS.consistent({p: list(range(first, first + n_img)) for p in range(1, count + 1)})


# ----------------------------------------------------------------------------------------
# the goldens, end to end
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["bin", "txt"])
@pytest.mark.parametrize("scene", VS.SCENES)
def test_goldens_end_to_end(scene, form, tmp_path):
    folder = os.path.join(VS.GOLDEN, scene, form)
    out = view_selection.select(folder, str(tmp_path), VS.BLOCK_SIZE, VS.OVERLAP)
    model = sparse_model.load(folder)
    pairs, block_list, border = VS.select(model, VS.BLOCK_SIZE, VS.OVERLAP)
    assert (out["viewpair"], out["blocks"], out["border"]) == (pairs, block_list, border)
    mine = VS.texts(pairs, block_list, border)
    text = {n: open(out["files"][n]).read() for n in mine}
    assert text == mine
    want = VS.canonical_pairs(VS.golden(scene, "viewpair.txt"))
    got = VS.canonical_pairs(text["viewpair"])
    assert sorted(got) == sorted(want) and len(want) == 20
    for view in want:
        assert got[view] == want[view], view
    assert VS.canonical_blocks(text["blocks"]) == VS.canonical_blocks(VS.golden(scene, "blocks.txt"))
    assert text["scene_border"] == VS.golden(scene, "scene_border.txt")
    # sources by score descending then id ascending, views by id ascending
    for r, src in pairs:
        assert src == sorted(src, key=lambda e: (-e[1], e[0]))
    assert [r for r, _ in pairs] == sorted(r for r, _ in pairs)


# ----------------------------------------------------------------------------------------
# hand-made models
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_img", [1, 3, 4, 5])
def test_the_seen_boundary(n_img):
    want = _check(_ring(n_img, 12))
    assert all(v["seen"] == n_img - 1 for v in want.values())
    assert all(len(v["sources"]) == n_img - 1 and v["max"] == (12 if n_img > 1 else 0) for v in want.values())
    # listing: select() on such a model lists a view iff it sees 3 others
    m = _ring(n_img, 12)
    h = view_selection.score(m, m.image_ids).host()
    assert ((h["seen"] >= view_selection.MIN_SEEN).all()) == (n_img >= 4)


def test_counts_of_exactly_10_and_11_and_the_tenth_of_the_maximum():
    # image 1 shares 10 points with image 2, 11 with image 3, and nothing else
    want = _check(VS.consistent({**{p: [1, 2] for p in range(1, 11)}, **{p: [1, 3] for p in range(11, 22)}}))
    assert want[1]["sources"] == [(3, 11, 11)] and want[1]["seen"] == 2 and want[2]["sources"] == []
    # max = 110 (image 2): a candidate at 11 is out (110 > 110 fails), one at 12 is in
    tracks = {p: [1, 2] for p in range(1, 111)}
    tracks.update({p: [1, 3] for p in range(200, 211)})
    tracks.update({p: [1, 4] for p in range(300, 312)})
    want = _check(VS.consistent(tracks))
    assert want[1]["max"] == 110 and want[1]["sources"] == [(2, 110, 110), (4, 12, 12)] and want[1]["seen"] == 3
    assert want[3]["sources"] == [(1, 11, 11)]


def test_images_without_observations_tracks_of_one_and_multiplicity():
    images = {1: [7, 7, 8], 2: [7, 8], 3: [], 4: [-1, -1, -1], 5: [9]}
    points = {7: ((0, 0, 0), [1, 2, 2, 1]), 8: ((1, 0, 0), [2, 1]), 9: ((2, 0, 0), [5])}   # 7: image 1 twice on both sides
    m = VS.make_model(images, points)
    want = _check(m)
    C = VS.rows(m, 1)[0]
    assert C == {1: 5, 2: 5} and VS.rows(m, 2)[0] == {1: 3, 2: 3}       # 2 observations x 2 entries = 4, plus point 8
    assert want[3] == want[4] == {"seen": 0, "max": 0, "sources": []} and want[5]["seen"] == 0
    # the same with counts past the threshold: twelve such points
    images = {1: [p for p in range(1, 13) for _ in range(2)], 2: list(range(1, 13))}
    m = VS.make_model(images, {p: ((0, 0, 0), [1, 2, 2, 1]) for p in range(1, 13)})
    assert _check(m)[1]["sources"] == [(2, 48, 48)]


@pytest.mark.parametrize("n_img", [65, 130])
def test_strides_ragged_tails_and_rows_that_are_no_multiple_of_a_wave(n_img):
    # image 1 has 700 observations (a 256-lane workgroup strides three times, the last ragged); image k sees the first
    # 10 (k // 2) + 3 of them (mod 400), so neighbours tie and the id breaks the tie, and both thresholds remove candidates
    tracks = {p: [1] + [k for k in range(2, n_img + 1) if p <= (10 * (k // 2) + 3) % 400] for p in range(1, 701)}
    m = VS.consistent(tracks)
    want = _check(m)
    assert m.img_offset[1] - m.img_offset[0] == 700 and want[1]["seen"] == n_img - 1
    assert 0 < len(want[1]["sources"]) < n_img - 1 and any(a[1] == b[1] for a, b in zip(want[1]["sources"], want[1]["sources"][1:]))
    # refs: a strict subset, not ascending, one image twice
    refs = [int(i) for i in (m.image_ids[-1], 1, m.image_ids[n_img // 2], 2, 1)]
    _check(m, refs)
    _check(m, [])


@pytest.mark.parametrize("mode", view_selection.MODES)
def test_the_scratch_path_equals_the_lds_path(mode):
    m = sparse_model.load(os.path.join(VS.GOLDEN, "dense", "bin"))
    assert m.n_img == 21
    a = view_selection.score(m, m.image_ids, mode).host()
    b = view_selection.score(m, m.image_ids, mode, lds_images=16).host()     # 21 (or 42) counters do not fit in 16
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert len(a["src"]) > 50          # the scene has sources to compare
    _check(m, m.image_ids.tolist()[::4], mode, lds_images=16)
    with pytest.raises(ValueError, match="lds_images"):
        view_selection.score(m, m.image_ids, mode, lds_images=view_selection.lds_images() + 1)


def test_more_reference_images_than_a_scratch_batch():
    m = VS.strip_flight(12, 100, 60, seed=3)       # 1200 images: two batches of rows on the scratch path
    assert m.n_img == 1200
    a = view_selection.score(m, m.image_ids).host()
    b = view_selection.score(m, m.image_ids, lds_images=0).host()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    _check(m, m.image_ids.tolist()[::97] + [1200], lds_images=0)


# ----------------------------------------------------------------------------------------
# angle mode
# ----------------------------------------------------------------------------------------
def _angle_model(thetas, count=12, extra=None):
    """Image 1 at (0, 0, 10) and image k + 2 at the angle thetas[k] (degrees) from it as seen from the origin, all seeing the same
    `count` points at the origin."""
    centers = {1: (0.0, 0.0, 10.0)}
    for k, t in enumerate(thetas):
        centers[k + 2] = (10.0 * np.sin(np.deg2rad(t)), 0.0, 10.0 * np.cos(np.deg2rad(t)))
    centers.update(extra or {})
    ids = sorted(centers)
    return VS.consistent({p: ids for p in range(1, count + 1)}, xyz={p: (0.0, 0.0, 0.0) for p in range(1, count + 1)}, centers=centers)


def test_angle_mode_at_the_bin_edges_and_around_theta0():
    edge, w = view_selection.angle_table()
    thetas = [4.94, 4.96, 5.04, 5.06, 0.05, 0.15, 29.99, 30.01, 179.94, 90.0]
    m = _angle_model(thetas)
    want = _check(m, mode="angle")
    S = VS.rows(m, 1, "angle")[1]
    assert S[2] == 12 * int(w[49]) and S[4] == 12 * int(w[50]) and S[10] == 0 and S[6] == 12 * int(w[0])
    assert len({S[k] for k in (2, 3, 4, 5)}) >= 2 and S[8] != S[9]              # both sides of an edge give different bins
    assert want[1]["max"] == 12 * 1024 and [s for s, _, _ in want[1]["sources"]][:2] == [4, 5]
    # a non-default table moves the peak
    want = _check(m, mode="angle", angle=(30.0, 2.0, 3.0))
    assert [s for s, _, _ in want[1]["sources"]][0] in (8, 9)
    assert _check(m, mode="points")[1]["sources"][0] == (2, 12, 12)


def test_angle_mode_a_point_between_two_cameras_and_a_point_at_a_centre():
    # image 2 straight behind the point (180 degrees), image 3 at the point itself (weight 0), image 4 at 5 degrees
    m = _angle_model([5.02], extra={3: (0.0, 0.0, -10.0), 4: (0.0, 0.0, 0.0)})
    want = _check(m, mode="angle")
    S = VS.rows(m, 1, "angle")[1]
    assert S == {2: 12 * 1024, 3: 0, 4: 0} and want[1]["sources"] == [(2, 12 * 1024, 12)] and want[1]["seen"] == 3
    assert VS.rows(m, 4, "angle")[1] == {1: 0, 2: 0, 3: 0}                       # the reference image at the point: every weight 0
    # exact bits on a model with real geometry, and S / 1024 in the file
    g = sparse_model.load(os.path.join(VS.GOLDEN, "sparse", "bin"))
    _check(g, mode="angle")
    _check(VS.strip_flight(3, 9, 50, seed=5), mode="angle")


def test_angle_mode_end_to_end(tmp_path):
    folder = os.path.join(VS.GOLDEN, "sparse", "txt")
    out = view_selection.select(folder, str(tmp_path), VS.BLOCK_SIZE, VS.OVERLAP, mode="angle", angle=(8, 2, 12))
    pairs, block_list, border = VS.select(sparse_model.load(folder), VS.BLOCK_SIZE, VS.OVERLAP, None, "angle", (8, 2, 12))
    assert {n: open(out["files"][n]).read() for n in out["files"]} == VS.texts(pairs, block_list, border)
    assert any(v != int(v) for _, src in pairs for _, v in src)


# ----------------------------------------------------------------------------------------
# blocks
# ----------------------------------------------------------------------------------------
def _mask(model, blocks):
    got = view_selection.block_references(model, blocks)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (len(blocks), model.n_img)
    got = got.cpu().numpy()
    assert set(np.unique(got).tolist()) <= {0, 1} and np.array_equal(got.astype(bool), VS.references(model, blocks))
    return got


def test_block_edges_overlaps_empty_blocks_and_a_given_border(tmp_path):
    xyz = {1: (10.0, 5.0, 0.0),       # exactly on the low x edge of block 0: the strict test excludes it
           2: (10.5, 5.0, 1e9),       # inside block 0; z is not tested
           3: (19.5, 5.0, 0.0),       # in the overlap of blocks 0 and 1
           4: (20.0, 5.0, 0.0),       # on the high edge of block 0, inside block 1
           5: (45.0, 5.0, 0.0),       # in no block
           6: (np.nextafter(10.0, 11.0), np.nextafter(10.0, 0.0), 0.0)}     # one ulp inside both edges
    m = VS.make_model({k: [k] for k in range(1, 7)}, {**{p: (xyz[p], [p]) for p in xyz}, -4: ((10.5, 5.0, 0.0), [1]), 0: ((10.5, 5.0, 0.0), [5])})
    blocks = [[10.0, 20.0, 0.0, 10.0, -1.0, 1.0], [19.0, 30.0, 0.0, 10.0, -1.0, 1.0], [30.0, 40.0, 0.0, 10.0, -1.0, 1.0]]
    got = _mask(m, blocks)
    assert got.tolist() == [[0, 1, 1, 0, 0, 1], [0, 0, 1, 1, 0, 0], [0, 0, 0, 0, 0, 0]]      # ids <= 0 name images 1 and 5: ignored
    assert _mask(m, []).shape == (0, 6)
    # a track names its images many times; a point in many blocks; more points than one workgroup
    big = VS.strip_flight(4, 12, 80, seed=2)
    bl, _ = view_selection.scene_blocks(big, base_size=[150, 120, 10], overlap=30)
    assert len(bl) > 8 and big.n_pts > 600
    _mask(big, bl)
    # end to end: the block no view enters is dropped, a given border is written as given
    m = VS.consistent({p: [1, 2, 3, 4] if p <= 12 else [5, 6, 7, 8] for p in range(1, 25)},
                      xyz={p: (5.0 + (p % 3), 5.0, float(p)) if p <= 12 else (25.0 + (p % 3), 5.0, float(p)) for p in range(1, 25)})
    VS.write_text(m, str(tmp_path / "in"))
    out = view_selection.select(str(tmp_path / "in"), str(tmp_path / "out"), block_size=[10, 10, 10], overlap=0, border=[0, 30, 0, 10, -5, 5])
    pairs, block_list, border = VS.select(m, [10, 10, 10], 0, [0, 30, 0, 10, -5, 5])
    assert (out["viewpair"], out["blocks"], out["border"]) == (pairs, block_list, border) and border == [0.0, 30.0, 0.0, 10.0, -5.0, 5.0]
    assert [views for _, views in block_list] == [[1, 2, 3, 4], [5, 6, 7, 8]] and len(view_selection.scene_blocks(m, [10, 10, 10], 0, border)[0]) == 3
    assert open(out["files"]["scene_border"]).read() == "0.0\n30.0\n0.0\n10.0\n-5.0\n5.0\n"


# ----------------------------------------------------------------------------------------
# what must not matter
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", view_selection.MODES)
def test_shuffles_change_nothing(mode, tmp_path):
    folder = os.path.join(VS.GOLDEN, "sparse", "bin")
    m = sparse_model.load(folder)
    rng = np.random.default_rng(7)
    s = VS.shuffled(m, 8)                                       # the observations within an image, the entries within a track
    VS.write_text(s, str(tmp_path / "s"), image_order=rng.permutation(m.n_img), point_order=rng.permutation(m.n_pts))   # images, points
    t = sparse_model.load(str(tmp_path / "s"))
    assert np.array_equal(t.image_ids, m.image_ids) and not np.array_equal(t.obs_point, m.obs_point) and not np.array_equal(t.trk_image, m.trk_image)
    a, b = view_selection.score(m, m.image_ids, mode).host(), view_selection.score(t, t.image_ids, mode).host()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    blocks, _ = view_selection.scene_blocks(m, VS.BLOCK_SIZE, VS.OVERLAP)
    assert torch.equal(view_selection.block_references(m, blocks), view_selection.block_references(t, blocks))
    outs = [view_selection.select(f, str(tmp_path / n), VS.BLOCK_SIZE, VS.OVERLAP, mode=mode) for n, f in (("a", folder), ("b", str(tmp_path / "s")))]
    for n in outs[0]["files"]:
        assert open(outs[0]["files"][n]).read() == open(outs[1]["files"][n]).read(), n


# ----------------------------------------------------------------------------------------
# the command line
# ----------------------------------------------------------------------------------------
def test_the_command_line_writes_the_three_files_and_the_json(tmp_path):
    folder = os.path.join(VS.GOLDEN, "sparse", "bin")
    cmd = [sys.executable, "-m", "deep3d_aerial_amd.view_selection", "--sparse", folder, "--out", str(tmp_path / "block"), "--block_size", "200,200,50",
           "--overlap", "4", "--json", str(tmp_path / "log" / "run.json")]
    res = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    log = json.loads((tmp_path / "log" / "run.json").read_text())
    assert json.loads(res.stdout.strip().split("\n")[-1]) == log
    assert (log["images"], log["blocks"], log["views"], log["score"], log["angle"]) == (21, 4, 20, "points", None)
    pairs, block_list, border = VS.select(sparse_model.load(folder), VS.BLOCK_SIZE, VS.OVERLAP)
    assert {n: open(log["files"][n]).read() for n in log["files"]} == VS.texts(pairs, block_list, border)
    assert log["sources"] == sum(len(s) for _, s in pairs) and log["border"] == border
    # in process: the other flags
    out = view_selection.main(["--sparse", folder, "--out", str(tmp_path / "b2"), "--score", "angle", "--angle", "8,2,12", "--border", "0,400,0,400,0,40"])
    pairs, block_list, border = VS.select(sparse_model.load(folder), None, 1.0, [0, 400, 0, 400, 0, 40], "angle", (8, 2, 12))
    assert (out["viewpair"], out["blocks"], out["border"]) == (pairs, block_list, border)
    with pytest.raises(SystemExit):
        view_selection.main(["--sparse", folder, "--out", str(tmp_path / "b3"), "--json", "log.txt"])
