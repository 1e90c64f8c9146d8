"""The view selection (csrc/view_select.hip, deep3d_aerial_amd/view_selection.py) on a synthetic strip flight
(tests/view_selection_scene.strip_flight: nadir cameras on parallel strips, a ground point seen by the cameras whose footprint
holds it), at two sizes.  Per size, device-event ms (one warm-up, then --runs timed calls, each on its own events: median, min,
max) of

  * the blocks kernel (d3d_view_select_blocks, its clear of the mask included) on the default 2 x 2 blocks;
  * the rows kernel (d3d_view_select_rows) over every image as a reference image, in both modes, with the counters in LDS and
    -- lds_images = 0 -- in the scratch rows (clear of the rows included);
  * the whole score() call (host checks, the segments, the launch, the compaction and the two sorts, the read);
  * a torch formulation of the same counts: every (observation, track entry) pair expanded to an index r n_img + s (gathers and
    repeat_interleave) and counted with torch.bincount into a dense [n_img, n_img] matrix, the expansion and the count timed
    apart; its row maxima must equal the kernel's.  Skipped with the error's text where it does not run (memory).

--reference DIR times, on the CPU and without a GPU, the reference's calculate_src_images_score_based_triangulated_points
(imported in place from DIR/pycolmap/view_selection.py) over every image of the small size only, and checks that it lists the
sources the restatement lists.  What bounds the kernels is not measured here: no kernel trace and no counters are taken.

    python tools/view_selection_bench.py [--runs 5] [--sizes small,large] [--out profiles/view_selection_bench.txt]
    python tools/view_selection_bench.py --reference /path/to/reference [--out ...]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import view_selection_scene as VS  # noqa: E402

SIZES = {"small": (20, 50, 1000), "large": (100, 100, 6450)}   # strips, images a strip, points an image


def stats(ms):
    ms = sorted(ms)
    return {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1]}


def timed(call, runs):
    import bench_common   # (needs torch: not for --reference)

    return stats(bench_common.timed(call, runs))


def torch_counts(d, n_img):
    """(C [n_img, n_img] int64, expansion ms, count ms): the dense co-visibility counts by torch alone."""
    import torch

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    obs_p = d["obs_point"].long()
    has = obs_p >= 0
    image_of_obs = torch.repeat_interleave(torch.arange(n_img, device=obs_p.device), d["img_offset"][1:] - d["img_offset"][:-1])
    obs_p, image_of_obs = obs_p[has], image_of_obs[has]
    first = d["trk_offset"][obs_p]
    length = d["trk_offset"][obs_p + 1] - first
    owner = torch.repeat_interleave(torch.arange(obs_p.shape[0], device=obs_p.device), length)
    start = torch.cumsum(length, 0) - length
    entry = first[owner] + (torch.arange(owner.shape[0], device=obs_p.device) - start[owner])
    index = image_of_obs[owner] * n_img + d["trk_image"][entry].long()
    ev[1].record()
    C = torch.bincount(index, minlength=n_img * n_img).reshape(n_img, n_img)
    ev[2].record()
    torch.cuda.synchronize()
    return C, ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])


def note(text):
    print("[view_selection_bench] " + text, file=sys.stderr, flush=True)


def gpu(sizes, runs, lines):
    import torch

    from deep3d_aerial_amd import view_selection as V

    out = {}
    for name in sizes:
        t0 = time.time()
        model = VS.strip_flight(*SIZES[name], seed=0)
        d, dev = V._device(model)
        pairs = model.pairs_per_image()
        row = {"images": model.n_img, "points": model.n_pts, "observations": int(model.img_offset[-1]), "pairs": int(pairs.sum()),
               "host_build_s": time.time() - t0}
        note("%s: model built and on the device after %.1f s" % (name, row["host_build_s"]))
        blocks, _ = V.scene_blocks(model)
        row["blocks_ms"] = timed(lambda: V.block_references(model, blocks), runs)
        room = np.minimum(pairs // (V.MIN_COUNT + 1), model.n_img - 1).astype(np.int64)
        seg = np.concatenate([[0], np.cumsum(room)]).astype(np.int64)
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        refs_k, seg_d = put(np.arange(model.n_img, dtype=np.int32)), put(seg)
        edge, weight = V.angle_table()
        table = (put(edge), put(weight.view(np.int32)))
        row["source_slots"] = int(seg[-1])
        for mode in V.MODES:
            for path, lds in (("lds", V.lds_images()), ("scratch", 0)):
                call = lambda: V._rows(model, d, dev, refs_k, seg_d, int(seg[-1]), table if mode == "angle" else None, lds)
                row["rows_%s_%s_ms" % (mode, path)] = timed(call, runs)
                note("%s: rows %s %s %.3f ms" % (name, mode, path, row["rows_%s_%s_ms" % (mode, path)]["median"]))
            t1 = time.time()
            got = V.score(model, model.image_ids, mode).host()
            row["score_%s_call_s" % mode] = time.time() - t1
            row["sources_%s" % mode] = int(len(got["src"]))
            if mode == "points":
                kernel_max = got["max"]
        note("%s: score() calls done" % name)
        try:
            torch_counts(d, model.n_img)   # warm-up
            C, expand_ms, count_ms = torch_counts(d, model.n_img)
            C.fill_diagonal_(0)
            row["torch_expand_ms"], row["torch_bincount_ms"] = expand_ms, count_ms
            row["torch_matches_kernel_max"] = bool(np.array_equal(C.max(1).values.cpu().numpy(), kernel_max))
            del C
        except RuntimeError as e:
            row["torch_error"] = str(e).split("\n")[0][:200]
        torch.cuda.empty_cache()
        out[name] = row
        lines.append("%s: %d images, %d points, %d observations, %d (observation, track entry) pairs, %d source slots" %
                     (name, row["images"], row["points"], row["observations"], row["pairs"], row["source_slots"]))
        for k in sorted(row):
            if k.endswith("_ms") and isinstance(row[k], dict):
                lines.append("  %-28s median %10.3f  min %10.3f  max %10.3f" % (k, row[k]["median"], row[k]["min"], row[k]["max"]))
        for k in ("torch_expand_ms", "torch_bincount_ms", "torch_matches_kernel_max", "torch_error", "score_points_call_s", "score_angle_call_s",
                  "sources_points", "sources_angle", "host_build_s"):
            if k in row:
                lines.append("  %-28s %s" % (k, row[k] if not isinstance(row[k], float) else "%.3f" % row[k]))
    return out


def reference(folder, lines):
    sys.path.insert(0, folder)
    from pycolmap import read_write_model as rw  # the reference, imported in place
    from pycolmap.view_selection import calculate_src_images_score_based_triangulated_points as ref_score

    model = VS.strip_flight(*SIZES["small"], seed=0)
    images = {}
    for k, i in enumerate(model.image_ids.tolist()):
        images[i] = rw.Image(id=i, qvec=model.qvec[k], tvec=model.tvec[k], camera_id=1, name=model.names[k], xys=None,
                             point3D_ids=model.obs_point[model.img_offset[k]:model.img_offset[k + 1]])
    points = {}
    for p, i in enumerate(model.point_ids.tolist()):
        points[i] = rw.Point3D(id=i, xyz=model.xyz[p], rgb=None, error=0.0, image_ids=model.trk_image[model.trk_offset[p]:model.trk_offset[p + 1]],
                               point2D_idxs=None)
    t0 = time.time()
    got = ref_score(model.image_ids.tolist(), images, points)
    seconds = time.time() - t0
    checked = 0
    for r, src in got[::37]:
        want = VS.view(model, int(r))
        assert sorted((int(s), int(c)) for s, c in src) == sorted((s, c) for s, c, _ in want["sources"]), r
        checked += 1
    lines.append("small: the reference's calculate_src_images_score_based_triangulated_points on the CPU, %d images, %d points: %.3f s "
                 "(%d views listed; %d of them compared with the restatement)" % (model.n_img, model.n_pts, seconds, len(got), checked))
    return {"reference_small_s": seconds, "listed": len(got)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sizes", default="small,large")
    ap.add_argument("--reference", default=None, help="the reference's folder: time its CPU function at the small size (no GPU needed)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    lines = []
    result = reference(a.reference, lines) if a.reference else gpu([s for s in a.sizes.split(",") if s], a.runs, lines)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + json.dumps(result) + "\n")
    print(text + json.dumps(result))
    return result


if __name__ == "__main__":
    main()
