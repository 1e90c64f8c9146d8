"""CPU checks of the view selection: the readers of the sparse model, the restatement of the rule against the
files the reference wrote for the two golden scenes (tests/golden/make_golden_view_selection.py), the writers, every refusal,
and the new entry points of the header."""
import os
import struct

import numpy as np
import pytest

import view_selection_scene as VS
from deep3d_aerial_amd import _lib, dataset, sparse_model, view_selection

FIELDS = ("image_ids", "qvec", "tvec", "img_offset", "obs_point", "point_ids", "xyz", "trk_offset", "trk_image")


def _load(scene, form):
    return sparse_model.load(os.path.join(VS.GOLDEN, scene, form))


@pytest.fixture(scope="module")
def restated():
    """scene -> (model, pairs, block list, border) by the restatement: computed once, shared, never changed."""
    out = {}
    for scene in VS.SCENES:
        model = _load(scene, "bin")
        out[scene] = (model,) + VS.select(model, VS.BLOCK_SIZE, VS.OVERLAP)
    return out


@pytest.mark.parametrize("scene", VS.SCENES)
def test_text_and_binary_readers_give_identical_records(scene):
    a, b = _load(scene, "txt"), _load(scene, "bin")
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f
    assert a.names == b.names and a.n_img == 21 and a.names[0] == "003.jpg"
    assert a.image_ids.dtype == np.int64 and (np.diff(a.image_ids) > 0).all() and (np.diff(a.image_ids) > 1).any()
    assert (np.diff(a.point_ids) > 0).all() and (np.diff(a.point_ids) > 1).any()
    assert a.img_offset[-1] == len(a.obs_point) and a.trk_offset[-1] == len(a.trk_image) and (a.obs_point == -1).sum() == 2 * a.n_img
    # the two CSR forms describe one set of (image, point) incidences
    by_image = sorted((int(a.image_ids[k]), int(p)) for k in range(a.n_img) for p in a.obs_point[a.img_offset[k]:a.img_offset[k + 1]] if p > 0)
    by_point = sorted((int(i), int(a.point_ids[p])) for p in range(a.n_pts) for i in a.trk_image[a.trk_offset[p]:a.trk_offset[p + 1]])
    assert by_image == by_point
    # camera centres: an identity rotation and t = -C
    assert np.array_equal(a.centers(), -a.tvec)


def test_binary_is_preferred_when_both_forms_exist(tmp_path):
    m = VS.consistent({5: [1, 2], 9: [2, 4]})
    VS.write_text(m, str(tmp_path))
    assert sparse_model.load(str(tmp_path)).n_img == 3
    with open(str(tmp_path / "images.bin"), "wb") as f:   # one image, id 77, no 2-D point
        f.write(struct.pack("<Q", 1) + struct.pack("<i7di", 77, 1, 0, 0, 0, 0, 0, 0, 1) + b"a.jpg\0" + struct.pack("<Q", 0))
    with pytest.raises(ValueError, match="names image id 1"):   # images.bin wins, so the text tracks name unknown images
        sparse_model.load(str(tmp_path))
    os.remove(str(tmp_path / "points3D.txt"))
    with open(str(tmp_path / "points3D.bin"), "wb") as f:
        f.write(struct.pack("<Q", 1) + struct.pack("<Q3d3Bd", 4, 1.0, 2.0, 3.0, 0, 0, 0, 0.5) + struct.pack("<Q", 2) + struct.pack("<4i", 77, 0, 77, 1))
    got = sparse_model.load(str(tmp_path))
    assert got.image_ids.tolist() == [77] and got.names == ["a.jpg"] and got.trk_image.tolist() == [77, 77] and got.xyz.tolist() == [[1.0, 2.0, 3.0]]
    with pytest.raises(FileNotFoundError):
        sparse_model.load(str(tmp_path / "nowhere"))


def test_the_reader_sorts_by_id_and_keeps_the_files_order_within(tmp_path):
    m = VS.make_model({7: [30, -1, 10, 30], 2: [10], 4: []}, {30: ((1, 2, 3), [7, 7]), 10: ((4, 5, 6), [2, 7]), -3: ((7, 8, 9), [])})
    VS.write_text(m, str(tmp_path), image_order=[2, 0, 1], point_order=[2, 0, 1])
    got = sparse_model.load(str(tmp_path))
    for f in FIELDS:
        assert np.array_equal(getattr(got, f), getattr(m, f)), f
    obs_p, trk_k, p_first = got.dense()
    assert obs_p.tolist() == [1, 2, -1, 1, 2] and obs_p.dtype == np.int32 and trk_k.tolist() == [0, 2, 2, 2] and p_first == 1
    assert got.pairs_per_image().tolist() == [2, 0, 6]


@pytest.mark.parametrize("scene", VS.SCENES)
def test_the_restatement_matches_the_reference_files(scene, restated):
    model, pairs, block_list, border = restated[scene]
    mine = VS.texts(pairs, block_list, border)
    want, got = VS.canonical_pairs(VS.golden(scene, "viewpair.txt")), VS.canonical_pairs(mine["viewpair"])
    assert sorted(want) == sorted(got) and len(want) == 20 and 401 not in want
    for view in want:   # every view, none skipped
        assert got[view] == want[view], view
    # the block ranges to the digits the file carries, the views of a block as a set; the reference's block order
    assert VS.canonical_blocks(mine["blocks"]) == VS.canonical_blocks(VS.golden(scene, "blocks.txt")) and len(block_list) == 4
    assert mine["scene_border"] == VS.golden(scene, "scene_border.txt")
    # the module's host parts agree with the restatement: blocks, the table-free texts
    blocks, scene_border = view_selection.scene_blocks(model, VS.BLOCK_SIZE, VS.OVERLAP)
    assert (blocks, scene_border) == VS.blocks(model, VS.BLOCK_SIZE, VS.OVERLAP) and all(type(v) is float for b in blocks for v in b)
    assert view_selection.pair_text(pairs) == mine["viewpair"] and view_selection.block_text(block_list) == mine["blocks"]
    assert view_selection.border_text(border) == mine["scene_border"]


def test_the_goldens_exercise_both_thresholds_ties_and_an_unlisted_view(restated):
    by_count = by_max = ties = 0
    for scene in VS.SCENES:
        model = restated[scene][0]
        for r in model.image_ids.tolist():
            v, C = VS.view(model, r), VS.rows(model, r)[0]
            by_count += sum(1 for s in C if s != r and C[s] <= 10)
            by_max += sum(1 for s in C if s != r and C[s] > 10 and 10 * C[s] <= v["max"])
            ties += sum(1 for a, b in zip(v["sources"], v["sources"][1:]) if a[1] == b[1])
            assert (v["seen"] < 3) == (r == 401)
    assert by_count and by_max and ties


def test_blocks_follow_the_reference_arithmetic_with_its_quirks():
    m = VS.consistent({p: [1] for p in range(1, 202)}, xyz={p: (float(p - 1), 2.0 * (p - 1), 0.5 * (p - 1)) for p in range(1, 202)})
    blocks, border = view_selection.scene_blocks(m)                      # defaults: 2 x 2 blocks of half the percentile range
    assert border == [1.0, 199.0, 2.0, 398.0, 0.5, 99.5] and len(blocks) == 4
    assert blocks[0] == [0.0, 100.0, 1.0, 200.0, 0.5, 99.5] and blocks[1] == [99.0, 199.0, 1.0, 200.0, 0.5, 99.5]   # low side only
    assert blocks[2][:4] == [0.0, 100.0, 199.0, 398.0]                                                            # row-major: j then i
    given, gb = view_selection.scene_blocks(m, base_size=[60, 500, 1], overlap=2.5, border=[0, 100, -5, 5, -1000, 1000])
    assert gb == [0.0, 100.0, -5.0, 5.0, -1000.0, 1000.0] and len(given) == 2
    assert given[1] == [57.5, 120.0, -7.5, 495.0, 0.5, 99.5]                                                      # z from the percentiles
    assert (given, gb) == VS.blocks(m, [60, 500, 1], 2.5, [0, 100, -5, 5, -1000, 1000])


def test_the_writers_round_trip_through_the_dataset_readers(tmp_path, restated):
    _, pairs, block_list, border = restated["dense"]
    for name, text in (("viewpair", view_selection.pair_text(pairs)), ("blocks", view_selection.block_text(block_list))):
        (tmp_path / (name + ".txt")).write_text(text)
    metas = dataset.read_view_pair_text(str(tmp_path / "viewpair.txt"), 1)
    assert metas == [[r] + [s for s, _ in src] for r, src in pairs if src] and len(metas) == 20
    got = dataset.read_scene_blocks(str(tmp_path / "blocks.txt"))
    assert [b["refs"] for b in got] == [views for _, views in block_list]
    assert [b["scene_range"] for b in got] == [[float("%.4f" % v) for v in rng] for rng, _ in block_list]
    # a listed view without a source is written with 0, a count as 30.0000, an angle score with four digits
    assert view_selection.pair_text([(4, []), (9, [(4, 30.0), (2, 1234 / 1024.0)])]) == "2\n4\n0 \n9\n2 4 30.0000 2 1.2051 \n"
    assert view_selection.block_text([([1.0, 2.5, 3.0, 4.0, 5.0, 6.12345], [9, 4])]) == "1\n1.0000 2.5000 3.0000 4.0000 5.0000 6.1235 \n9 4 \n"
    assert view_selection.border_text([1, 2.5, 1e-7, 4, 5, 6]) == "1.0\n2.5\n1e-07\n4.0\n5.0\n6.0\n"


def test_the_angle_table():
    edge, w = view_selection.angle_table()
    assert edge.shape == (1800,) and edge.dtype == np.float64 and w.shape == (1800,) and w.dtype == np.uint32
    assert edge[0] == 1.0 and (np.diff(edge) < 0).all() and edge[-1] > -1.0
    assert w.max() == 1024 and int(w.argmax()) == 50 and w[49] == 1023 and w[1799] == 0      # the peak: the bin from 5 degrees on
    assert w[39] == round(1024 * np.exp(-(3.95 - 5) ** 2 / 2.0)) and w[150] == round(1024 * np.exp(-(15.05 - 5) ** 2 / 200.0))
    assert view_selection.angle_table(20, 2, 4)[1][200] == round(1024 * np.exp(-(20.05 - 20) ** 2 / 32.0))
    with pytest.raises(ValueError):
        view_selection.angle_table(5, 0, 10)
    # the restatement's two ways to find the bin agree, at the edges too
    c0, x = np.array([0.0, 0.0, 10.0]), np.zeros(3)
    for c in (1.0, np.nextafter(1.0, 2), edge[7], np.nextafter(edge[7], 1), np.nextafter(edge[7], -1), 0.0, -1.0, -1.5):
        slow = max([k for k in range(1800) if c <= edge[k]], default=0)
        assert VS._bin_fast(c, edge) == slow, c
    assert VS.weight(c0, np.array([0.0, 0.0, -10.0]), x, edge, w) == 0 and VS.weight(c0, x, x, edge, w) == 0
    assert VS.weight(c0, np.array([10 * np.tan(np.deg2rad(5.02)), 0.0, 10.0]), x, edge, w) == 1024


def test_every_refusal_of_the_reader(tmp_path, monkeypatch):
    ok = VS.make_model({1: [5, 6], 2: [5]}, {5: ((0, 0, 0), [1, 2]), 6: ((1, 1, 1), [1])})

    def written(model, name):
        folder = str(tmp_path / name)
        VS.write_text(model, folder)
        return folder

    assert sparse_model.load(written(ok, "ok")).n_pts == 2
    with pytest.raises(ValueError, match="image id 2 observes point id 8"):
        sparse_model.load(written(VS.make_model({1: [5], 2: [5, 8]}, {5: ((0, 0, 0), [1, 2])}), "absent_point"))
    assert sparse_model.load(written(VS.make_model({1: [5, 0, -7]}, {5: ((0, 0, 0), [1])}), "ids_below_one")).obs_point.tolist() == [5, 0, -7]
    with pytest.raises(ValueError, match="point id 6 names image id 3"):
        sparse_model.load(written(VS.make_model({1: [5], 2: [5]}, {5: ((0, 0, 0), [1, 2]), 6: ((0, 0, 0), [3])}), "unknown_image"))
    monkeypatch.setattr(sparse_model, "MAX_ENTRIES", 2)
    with pytest.raises(ValueError, match=r"3 observations, at most 2\^31 - 1"):
        sparse_model.load(str(tmp_path / "ok"))
    monkeypatch.setattr(sparse_model, "MAX_ENTRIES", (1 << 31) - 1)
    # truncated files, text and binary
    folder = written(ok, "cut_txt")
    text = open(os.path.join(folder, "images.txt")).read().rstrip("\n")
    open(os.path.join(folder, "images.txt"), "w").write(text[:text.rindex("\n") + 1].rstrip("\n"))      # the last image lost its second line
    with pytest.raises(ValueError, match="truncated: image id 2"):
        sparse_model.load(folder)
    folder = written(ok, "cut_points_txt")
    open(os.path.join(folder, "points3D.txt"), "w").write("5 0.0 0.0 0.0 0 0 0 0.5 1 0 2\n")
    with pytest.raises(ValueError, match="truncated: the track of point id 5"):
        sparse_model.load(folder)
    image = struct.pack("<i7di", 3, 1, 0, 0, 0, 0, 0, 0, 1) + b"a.jpg\0" + struct.pack("<Q", 2) + struct.pack("<ddq", 0, 0, -1) * 2
    point = struct.pack("<Q3d3Bd", 4, 1.0, 2.0, 3.0, 0, 0, 0, 0.5) + struct.pack("<Q", 1) + struct.pack("<2i", 3, 0)
    whole_i, whole_p = struct.pack("<Q", 1) + image, struct.pack("<Q", 1) + point
    assert (len(whole_i), len(whole_p)) == (134, 67)
    for name, keep_i, keep_p, what in (("a", 8 + 30, 67, "image 1 of 1"), ("b", 8 + 64 + 3, 67, "name of image id 3"),
                                       ("c", 8 + 64 + 6 + 4, 67, "number of 2-D points of image id 3"), ("d", 134 - 30, 67, "2-D points of image id 3"),
                                       ("e", 134, 8 + 20, "point 1 of 1"), ("f", 134, 8 + 43 + 3, "track length of point id 4"),
                                       ("g", 134, 67 - 4, "track of point id 4"), ("h", 4, 67, "image count")):
        folder = tmp_path / name
        folder.mkdir()
        (folder / "images.bin").write_bytes(whole_i[:keep_i])
        (folder / "points3D.bin").write_bytes(whole_p[:keep_p])
        with pytest.raises(ValueError, match="truncated.*" + what):
            sparse_model.load(str(folder))
    folder = tmp_path / "whole"
    folder.mkdir()
    (folder / "images.bin").write_bytes(whole_i)
    (folder / "points3D.bin").write_bytes(whole_p)
    assert sparse_model.load(str(folder)).obs_point.tolist() == [-1, -1]
    with pytest.raises(ValueError, match="image id 1 is given twice"):
        folder = written(ok, "twice")
        with open(os.path.join(folder, "images.txt"), "a") as f:
            f.write("1 1 0 0 0 0 0 0 1 again.jpg\n\n")
        sparse_model.load(folder)


def test_every_refusal_of_the_rule(monkeypatch):
    m = VS.consistent({5: [1, 2], 6: [1, 2]})
    with pytest.raises(ValueError, match="tie_points.*out of scope"):
        view_selection.score(m, [1], mode="tie_points")
    with pytest.raises(ValueError, match="mode must be one of"):
        view_selection.score(m, [1], mode="area")
    with pytest.raises(ValueError, match="refs names image id 3"):
        view_selection.score(m, [1, 3])
    with pytest.raises(ValueError, match="sigma"):
        view_selection.score(m, [1], mode="angle", angle=(5, -1, 10))
    monkeypatch.setattr(view_selection, "MAX_PAIRS", 4)
    with pytest.raises(ValueError, match=r"image id 1: .* 4 entries in all, at most 2\^22 - 1"):
        view_selection.score(m, [2])
    monkeypatch.undo()
    assert view_selection.MAX_PAIRS == 1 << 22
    with pytest.raises(ValueError, match="at most %d" % view_selection.max_blocks()):
        view_selection.block_references(m, [[0, 1, 0, 1, 0, 1]] * (view_selection.max_blocks() + 1))
    with pytest.raises(ValueError, match="no point"):
        view_selection.scene_blocks(VS.make_model({1: []}, {}))
    with pytest.raises(ValueError, match="six values"):
        view_selection.scene_blocks(m, border=[0, 1])
    with pytest.raises(TypeError):
        view_selection.block_references({"not": "a model"}, [])
    import torch

    if not torch.cuda.is_available():   # the GPU parts refuse to run anywhere else
        for call in (lambda: view_selection.score(m, [1]), lambda: view_selection.block_references(m, [[0, 1, 0, 1, 0, 1]])):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call()
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            view_selection.main(["--sparse", "x", "--out", "y"])


def test_the_header_declares_the_entry_points_and_the_abi_is_still_11():
    assert _lib.ABI_VERSION == 11 and _lib.CONSTANTS["D3D_VIEW_SELECT_MAX_BLOCKS"] == 512
    import ctypes

    for name, n_args, ret in (("d3d_view_select_lds_images", 0, ctypes.c_int), ("d3d_view_select_scratch_bytes", 4, ctypes.c_size_t),
                              ("d3d_view_select_blocks", 11, ctypes.c_int), ("d3d_view_select_rows", 28, ctypes.c_int)):
        args, got = _lib.PROTOTYPES[name]
        assert len(args) == n_args and got is ret, name
    assert sorted(_lib.STRUCTS) == ["d3d_mesh_grid_t", "d3d_mesh_view_t", "d3d_ortho_view_t"]   # no new struct
    _lib.build()
    lib = _lib.load()
    most = lib.d3d_view_select_lds_images()
    assert most * 4 <= 160 * 1024 and most >= 40000
    assert lib.d3d_view_select_scratch_bytes(5, 100, 0, most) == 256 and lib.d3d_view_select_scratch_bytes(5, 100, 1, 100) == 4096
    assert lib.d3d_view_select_scratch_bytes(5000, 100, 0, 16) == 1024 * 100 * 4 and lib.d3d_view_select_scratch_bytes(5, 100, 2, 16) == 0
    assert lib.d3d_view_select_scratch_bytes(5, 100, 0, most + 1) == 0
    # refusals come back as errors before any launch
    assert lib.d3d_view_select_blocks(None, None, None, 1, 0, 0, 4, None, 1, None, None) == -1 and b"null" in lib.d3d_last_error()
    assert lib.d3d_view_select_blocks(None, None, None, 0, 0, 0, 4, None, 513, None, None) == -1 and b"blocks" in lib.d3d_last_error()
    assert lib.d3d_view_select_rows(*([None, None, 0, None, None, 0, 0, 4, None, 1, 0] + [None] * 4 + [0, 16, None, 0, None, 0] + [None] * 7)) == -1
    assert b"null" in lib.d3d_last_error()
    assert lib.d3d_view_select_rows(*([None, None, 0, None, None, 0, 0, 4, None, 1, 7] + [None] * 4 + [0, 16, None, 0, None, 0] + [None] * 7)) == -1
    assert b"mode" in lib.d3d_last_error()


def test_the_strip_flight_model_is_consistent():
    m = VS.strip_flight(3, 8, 40, seed=1)
    assert m.n_img == 24 and m.img_offset[-1] == m.trk_offset[-1] > 0
    by_image = sorted((int(m.image_ids[k]), int(p)) for k in range(m.n_img) for p in m.obs_point[m.img_offset[k]:m.img_offset[k + 1]])
    by_point = sorted((int(i), int(m.point_ids[p])) for p in range(m.n_pts) for i in m.trk_image[m.trk_offset[p]:m.trk_offset[p + 1]])
    assert by_image == by_point
    c = m.centers()
    for p in range(0, m.n_pts, 7):   # a track is exactly the cameras whose footprint holds the point
        want = [int(m.image_ids[k]) for k in range(m.n_img) if abs(c[k, 0] - m.xyz[p, 0]) <= 75 and abs(c[k, 1] - m.xyz[p, 1]) <= 100]
        assert sorted(m.trk_image[m.trk_offset[p]:m.trk_offset[p + 1]].tolist()) == want
