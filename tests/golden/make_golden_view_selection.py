#!/usr/bin/env python3
"""Goldens of the view selection, made by RUNNING THE REFERENCE's own stage on two seeded synthetic nadir
scenes:

    python tests/golden/make_golden_view_selection.py

Per scene the model is written with the reference's pycolmap/read_write_model.write_model, as .txt and as .bin; then, as
run.py: select_view does, calculate_block_border, select_view_based_viewed_points(mode='triangulated_points') and the three
writers of IO/params_io.py run on it (on both forms: they must give the same files).  Only data is kept, under
tests/golden/view_selection/<scene>/: txt/ and bin/ with the model files, and viewpair.txt, blocks.txt, scene_border.txt.

A scene: a 4 x 5 grid of nadir cameras plus one isolated camera, image ids and point ids with gaps, ground points seen by a
camera with a probability that falls off with the distance, so that the overlaps are graded.  "sparse" has few points, so the `> 10` test removes
candidates; "dense" adds a patch of points between four cameras, so that the `max / 10` test removes distant candidates too.  Both
are cut to the fewest points at which the assertions below hold, to keep the committed files small.  The properties the tests lean on are asserted here.

What is bound for the import, and why it does not change what is pinned: IO/params_io.py imports cv2, matplotlib and the
reference's `format` package at module level and uses none of them in the three writers; they are bound to empty modules.
Nothing is copied: the modules are imported in place from D3D_REFERENCE."""
import os
import shutil
import sys
import tempfile
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("D3D_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

for name in ("cv2", "matplotlib", "matplotlib.pyplot", "format", "format.cameras"):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
sys.modules["format"].cameras = sys.modules["format.cameras"]
sys.path.insert(0, REF)

from IO.params_io import save_border_as_file, write_block_text, write_pair_text  # noqa: E402  (the reference)
from pycolmap import read_write_model as rw  # noqa: E402  (the reference)
from pycolmap.view_selection import calculate_block_border, select_view_based_viewed_points  # noqa: E402  (the reference)

import view_selection_scene as VS  # noqa: E402

OUT = os.path.join(HERE, "view_selection")
SCENES = {"sparse": (220, 11, (110.0, 90.0), 0), "dense": (300, 12, (110.0, 90.0), 330)}   # candidate points, seed, reach of a camera, extra points between four cameras
LIMIT = 1 << 20


def scene(n_candidates, seed, half, n_dense):
    """(cameras, images, points3D) in the reference's records."""
    rng = np.random.default_rng(seed)
    grid = [(50.0 + 100.0 * i, 40.0 + 80.0 * j) for j in range(5) for i in range(4)]
    ids = [3 + 7 * k for k in range(len(grid))] + [401]
    centers = [(x, y, 300.0) for x, y in grid] + [(200.0, 200.0, 900.0)]
    # a camera sees a point with a probability that falls off with the distance over `half`: graded overlaps
    xyz = np.stack([rng.uniform(0, 400, n_candidates), rng.uniform(0, 400, n_candidates), rng.normal(20, 4, n_candidates)], 1)
    # a textured patch between the first four cameras: their mutual counts pass ten times those of distant pairs
    xyz = np.concatenate([xyz, np.stack([rng.uniform(60, 140, n_dense), rng.uniform(40, 120, n_dense), rng.normal(20, 4, n_dense)], 1)])
    n_candidates += n_dense
    # the isolated camera: a handful of points of its own, two of which two grid cameras also saw (seen = 2)
    xyz = np.concatenate([xyz, np.stack([rng.uniform(150, 250, 12), rng.uniform(150, 250, 12), rng.normal(20, 4, 12)], 1)])
    own = np.arange(len(xyz)) >= n_candidates
    pid, point_ids = 5, []
    for _ in range(len(xyz)):
        point_ids.append(pid)
        pid += int(rng.integers(1, 4))
    obs = {i: [] for i in ids}
    points = {}
    for p, x, far in zip(point_ids, xyz, own):
        if far:
            track = [401] + ([ids[0], ids[1]] if p % 2 == 0 else [])
        else:
            track = [i for i, c in zip(ids[:-1], centers) if rng.random() < np.exp(-(((x[0] - c[0]) / half[0]) ** 2 + ((x[1] - c[1]) / half[1]) ** 2))]
        if len(track) < 2 and not far:
            continue
        for i in track:
            obs[i].append(p)
        points[p] = rw.Point3D(id=p, xyz=np.round(x, 1), rgb=np.array([128, 128, 128]), error=0.5, image_ids=np.array(track),
                               point2D_idxs=np.array([len(obs[i]) - 1 for i in track]))
    images = {}
    for i, c in zip(ids, centers):
        got = obs[i] + [-1, -1]   # two 2-D points without a 3-D point
        images[i] = rw.Image(id=i, qvec=np.array([1.0, 0.0, 0.0, 0.0]), tvec=-np.array(c), camera_id=1, name="%03d.jpg" % i,
                             xys=rng.integers(0, 10, (len(got), 2)).astype(np.float64), point3D_ids=np.array(got))
    cameras = {1: rw.Camera(id=1, model="PINHOLE", width=1000, height=1000, params=np.array([1000.0, 1000.0, 500.0, 500.0]))}
    return cameras, images, points


def reference_run(folder, out):
    ranges, border = calculate_block_border(folder, base_size=list(VS.BLOCK_SIZE), base_overlap=VS.OVERLAP)
    in_range, viewpair = select_view_based_viewed_points("", folder, ranges, mode="triangulated_points")
    os.makedirs(out, exist_ok=True)
    write_pair_text(os.path.join(out, "viewpair.txt"), viewpair)
    write_block_text(os.path.join(out, "blocks.txt"), in_range)
    save_border_as_file(os.path.join(out, "scene_border.txt"), border)
    return {n: open(os.path.join(out, n + ".txt")).read() for n in ("viewpair", "blocks", "scene_border")}


def main():
    for name, (n_candidates, seed, half, n_dense) in SCENES.items():
        cameras, images, points = scene(n_candidates, seed, half, n_dense)
        dst = os.path.join(OUT, name)
        shutil.rmtree(dst, ignore_errors=True)
        for ext in ("txt", "bin"):
            os.makedirs(os.path.join(dst, ext))
            rw.write_model(cameras, images, points, os.path.join(dst, ext), "." + ext)
        with tempfile.TemporaryDirectory() as tmp:
            got = reference_run(os.path.join(dst, "txt"), os.path.join(tmp, "txt"))
            assert got == reference_run(os.path.join(dst, "bin"), os.path.join(tmp, "bin")), "the two forms disagree"
            for n in got:
                shutil.copy(os.path.join(tmp, "txt", n + ".txt"), os.path.join(dst, n + ".txt"))
        # the properties the tests lean on, by the restatement
        model = VS.sparse_model.load(os.path.join(dst, "bin"))
        views = {int(i): VS.view(model, int(i)) for i in model.image_ids}
        C = {r: VS.rows(model, r)[0] for r in views}
        by_count = sum(1 for r in views for s in C[r] if s != r and 0 < C[r][s] <= 10)
        by_max = sum(1 for r, v in views.items() for s in C[r] if s != r and C[r][s] > 10 and 10 * C[r][s] <= v["max"])
        ties = sum(1 for v in views.values() for a, b in zip(v["sources"], v["sources"][1:]) if a[1] == b[1])
        unlisted = [r for r, v in views.items() if v["seen"] < 3]
        pairs, block_list, border = VS.select(model, VS.BLOCK_SIZE, VS.OVERLAP)
        print("%s: %d images, %d points, %d blocks, %d views; removed by >10: %d, by max/10: %d (max %d); ties %d; unlisted %r"
              % (name, model.n_img, model.n_pts, len(block_list), len(pairs), by_count, by_max, max(v["max"] for v in views.values()),
                 ties, unlisted))
        assert by_count >= 1 and ties >= 1 and unlisted == [401]
        assert by_max >= 1 or name != "dense", "the max/10 test must remove a candidate in the dense scene"
        assert VS.canonical_pairs(got["viewpair"]) == VS.canonical_pairs(VS.texts(pairs, block_list, border)["viewpair"])
        assert VS.canonical_blocks(got["blocks"]) == VS.canonical_blocks(VS.texts(pairs, block_list, border)["blocks"])
        for root, _, files in os.walk(dst):
            for f in files:
                size = os.path.getsize(os.path.join(root, f))
                assert size < LIMIT, (f, size)
                print("   %-28s %7.1f KiB" % (os.path.relpath(os.path.join(root, f), dst), size / 1024))


if __name__ == "__main__":
    main()
