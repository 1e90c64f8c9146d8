#!/usr/bin/env python3
"""Headline benchmark: fused homography-warp + variance cost volume (BASELINE.json config 2).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full [--no-cpu-baseline] [--no-secondary]]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

One "step" = one reference view: 5 views x 384 depth planes over 32 x 688 x 464 fp32 feature
maps (1/4-resolution features of a 2752 x 1856 image) -> the [32,384,688,464] variance
volume, through the C-ABI kernel d3d_variance_volume.  Inputs are synthetic (seeded N(0,1)
features, converging cameras, deep3d_aerial_amd/synthetic.py) and resident in HBM before the
timed region.  With N > 1 every rank sweeps its own reference views (independent work, no
collective on the data path): weak scaling, value = all ranks' voxels / max-over-ranks time.

A plain run does only what the headline needs: it sets up, warms up, times the steps, writes the outputs when
--dump-outputs is given and prints ONE JSON line on rank 0, including
  roofline      -- algorithmic HBM bytes per launch / mean kernel time from the timed steps' HIP events; `issue_floor_ms` =
                   what the plane loop's instruction stream alone costs on this chip (measured replay, see issue_floor_ms)
  per_rank      -- every rank's kernel time, wall time and device (N > 1 only).
--full also runs, after the timed steps, what the headline does not need, and adds it to the same line:
  parity        -- 16 planes of the volume just produced against the CPU oracle (N = 1 only)
  cpu_baseline  -- the CPU oracle (oracle/planesweep_oracle.c, OpenMP) timed on a bounded sample of the same workload on
                   the host's cores, and the reference's op sequence in plain PyTorch CPU (N = 1 only; --no-cpu-baseline
                   drops it and parity)
  secondary     -- BASELINE config 3: the three cascades per view, the predict strip, the regulariser and the cascade-stage
                   sweeps (N = 1 only; --no-secondary drops it)
  exchange      -- BASELINE config 5's all-gather of the depth / confidence maps (N > 1 only).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from deep3d_aerial_amd import config, ops, synthetic as S  # noqa: E402

V, C, D, H_FEAT, W_FEAT = 5, 32, 384, 688, 464
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)


# What the vector units and the LDS allow this formulation of the kernel: tools/sweep_sandbox.hip
# replays the plane loop's instruction stream -- geometry of 4 views, 64 `ds_read_b128` taps, blend + sum / sum of squares,
# 16 stores per 16-channel group -- with no planner, no staging and no barriers.  The cycles per (64 pixels x 1 plane x
# 16 channels) per SIMD are PARSED from the tool's committed raw output, and only while that file and the tool still hash to
# what profiles/issue_floor.json recorded (no hard-coded constants without a guard); the clock is the one
# the chip held in the committed counter profile of the same kernel source (GRBM_GUI_ACTIVE / 8 / kernel time).
SIMDS = 256 * 4


def issue_floor():
    """{'2_compute_waves_per_simd': ms, '3_compute_waves_per_simd': ms, 'clock_ghz': f, ...} or None when a guard fails."""
    import hashlib
    import re

    try:
        meta = json.load(open(os.path.join(ROOT, "profiles", "issue_floor.json")))
        sha = lambda rel: hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest()
        if sha(meta["source"]) != meta["source_sha256"] or sha(meta["tool"]) != meta["tool_sha256"]:
            return None
        text = open(os.path.join(ROOT, meta["source"])).read().split("== later run")[0]
        cyc = {int(m.group(1)): float(m.group(2)) for m in re.finditer(
            r"\+ taps \+ stores\s+waves/SIMD (\d) :\s+\d+ cycles per plane-group per wave,\s+(\d+) per SIMD", text)}
        clock, clock_src = float(meta["clock_ghz_fallback"]), "fallback (profiles/r03_pk_rate.txt)"
        traffic, info = profiled_traffic()
        if info and info.get("matches_current_source"):
            prof = json.load(open(os.path.join(ROOT, "profiles", "pmc_latest.json")))
            g = prof.get("sq_counters_per_launch", {}).get("GRBM_GUI_ACTIVE")
            if g and prof.get("kernel_trace_avg_ns"):
                clock, clock_src = g / 8.0 / prof["kernel_trace_avg_ns"], "GRBM_GUI_ACTIVE / 8 / kernel time of profiles/pmc_latest.json"
        groups_per_simd = (D * H_FEAT * W_FEAT / 64.0) * (C // 16) / SIMDS
        ms = lambda w: groups_per_simd * cyc[w] / (clock * 1e6)
        return {"2_compute_waves_per_simd": ms(2), "3_compute_waves_per_simd": ms(3), "clock_ghz": clock, "clock_source": clock_src,
                "cycles_per_group_per_simd": {"2": cyc[2], "3": cyc[3]}, "source": meta["source"], "source_sha256": meta["source_sha256"][:16]}
    except Exception:
        return None


def issue_floor_fields(kern_ms):
    f = issue_floor()
    if f is None:
        return {"issue_floor_ms": None}
    return {"issue_floor_ms": round(f["2_compute_waves_per_simd"], 3),
            "issue_floor": {"ms_at_3_compute_waves_per_simd": round(f["3_compute_waves_per_simd"], 3),
                            "clock_ghz": round(f["clock_ghz"], 3), "clock_source": f["clock_source"],
                            "cycles_per_group_per_simd": f["cycles_per_group_per_simd"],
                            "source": "tools/sweep_sandbox.hip replay of the plane loop (taps + arithmetic + stores, nothing else), "
                                      + f["source"] + " (sha256 " + f["source_sha256"] + ", guarded by profiles/issue_floor.json)",
                            "kernel_over_floor": round(kern_ms / f["2_compute_waves_per_simd"], 3)}}


def algorithmic_bytes():
    """read V feature maps once + write the fp32 volume once."""
    reads = V * C * H_FEAT * W_FEAT * 4
    writes = C * D * H_FEAT * W_FEAT * 4
    return reads + writes


def host_threads():
    """Host cores this process may actually use: affinity mask, capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return max(1, n)


def torch_cpu_leg(proj_host, feats_host, depth_host, threads, budget_s=6.0):
    """The reference's own op sequence (module.py:516-557 + cas_mvsnet.py:46-60) written in this harness with plain
    PyTorch CPU operators -- inverse/matmul, the pixel grid, F.grid_sample(bilinear, zeros, align_corners=True), sum and
    sum of squares -- in chunks of 8 planes (the full 384-plane call needs ~50 GB of host memory), on a
    bounded number of chunks.  Nothing of the reference is imported: this is the baseline a user of the reference's
    CPU path would see on this box's host cores."""
    import torch.nn.functional as F

    old = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        feats = [torch.from_numpy(f)[None] for f in feats_host]             # [1,C,h,w]
        projs = [torch.from_numpy(p)[None] for p in proj_host]              # [1,4,4]
        ref, ref_proj = feats[0], projs[0]
        h, w = H_FEAT, W_FEAT
        V = len(feats)

        def warp(src_fea, src_proj, dvals):
            nd = dvals.shape[1]
            proj = torch.matmul(src_proj, torch.inverse(ref_proj))
            rot, trans = proj[:, :3, :3], proj[:, :3, 3:4]
            y, x = torch.meshgrid([torch.arange(0, h, dtype=torch.float32), torch.arange(0, w, dtype=torch.float32)], indexing="ij")
            xyz = torch.stack((x.reshape(-1), y.reshape(-1), torch.ones(h * w)))[None]
            rot_depth_xyz = torch.matmul(rot, xyz).unsqueeze(2).repeat(1, 1, nd, 1) * dvals.view(1, 1, nd, -1)
            pxyz = rot_depth_xyz + trans.view(1, 3, 1, 1)
            pxy = pxyz[:, :2] / pxyz[:, 2:3]
            grid = torch.stack((pxy[:, 0] / ((w - 1) / 2) - 1, pxy[:, 1] / ((h - 1) / 2) - 1), dim=3)
            out = F.grid_sample(src_fea, grid.view(1, nd * h, w, 2), mode="bilinear", padding_mode="zeros", align_corners=True)
            return out.view(1, C, nd, h, w)

        def chunk(d0):
            dvals = torch.from_numpy(depth_host[d0:d0 + 8])[None]
            vol = ref.unsqueeze(2).repeat(1, 1, 8, 1, 1)
            vsum, vsq = vol, vol ** 2
            for i in range(1, V):
                wv = warp(feats[i], projs[i], dvals)
                vsum = vsum + wv
                vsq = vsq + wv ** 2
            return vsq.div_(V).sub_(vsum.div_(V).pow_(2))

        with torch.no_grad():
            t0 = time.perf_counter()
            chunk(D // 2)
            first = time.perf_counter() - t0
            n = int(max(1, min(6, budget_s / max(first, 1e-3))))
            t0 = time.perf_counter()
            for k in range(n):
                chunk((D // 2 + 8 * (k + 1)) % (D - 8))
            dt = time.perf_counter() - t0
        return {"value": round(n * 8 * h * w / dt / 1e6, 3), "unit": "Mvoxels/s", "cores": threads, "kind": "torch-ops",
                "sample": "%d chunks of 8 planes of the same 5-view 32x688x464 workload, %.1f s" % (n, dt)}
    finally:
        torch.set_num_threads(old)


def cpu_baseline(proj34_host, feats_host, depth_host, gpu_volume=None):
    """Times the CPU oracle on a depth sub-range of the same workload (bounded to ~10-20 s).  The planes the oracle
    computed are then compared with the same planes of the volume the timed kernel left in HBM (outside every timed
    region): BASELINE.json's "L1 vs ref" half of the metric, at the cost-volume level, at full size."""
    import oracle

    oracle.build()
    cores = host_threads()
    oracle.set_num_threads(cores)
    probe = 4
    t0 = time.perf_counter()
    oracle.variance_volume(feats_host[0], feats_host[1:], proj34_host, depth_host[:probe])
    dt = time.perf_counter() - t0
    planes = int(min(D, max(probe, probe * 12.0 / max(dt, 1e-3))))
    start = (D - planes) // 2
    t0 = time.perf_counter()
    want = oracle.variance_volume(feats_host[0], feats_host[1:], proj34_host, depth_host[start:start + planes])
    dt = time.perf_counter() - t0
    vox = planes * H_FEAT * W_FEAT
    cb = {"value": round(vox / dt / 1e6, 3), "unit": "Mvoxels/s", "cores": oracle.num_threads(), "kind": "port",
          "sample": "%d of %d depth planes (planes %d..%d) of the same 5-view 32x688x464 workload, %.1f s"
                    % (planes, D, start, start + planes - 1, dt)}
    parity = None
    if gpu_volume is not None:
        # up to 16 of the oracle's planes, evenly spread over its range (16 planes = 654 MB of device-to-host copy)
        sel = np.unique(np.linspace(0, planes - 1, min(planes, 16)).round().astype(np.int64))
        got = gpu_volume[:, torch.from_numpy(start + sel).to(gpu_volume.device)].cpu().numpy()
        ref = np.ascontiguousarray(want[:, sel])
        num = float(np.abs(got - ref).mean(dtype=np.float64))
        den = float(np.abs(ref).mean(dtype=np.float64))
        parity = {"variance_rel_l1": num / max(den, 1e-30), "variance_max_abs": float(np.abs(got - ref).max()),
                  "planes": [int(start + k) for k in sel], "voxels": int(sel.size * H_FEAT * W_FEAT),
                  "tolerance_rel_l1": 5e-5, "against": "oracle/planesweep_oracle.c (restates module.py:516-557 + cas_mvsnet.py:45-60)",
                  "ok": bool(num / max(den, 1e-30) < 5e-5)}
    return cb, parity


DUMP_SAMPLE_VOXELS = 1 << 22   # seeded uniform sample of the volume (16 MB)
DUMP_SAMPLE_SEED = 20240607


def dump_outputs(out_dir, volume):
    """What the timed path handed its caller in the last step -- the [C, D, h, w] fp32 variance volume (15.7 GB at the
    headline size) -- as .npy files of at most ~58 MB: the whole middle depth plane [C, h, w] and a fixed, seeded sample of
    voxels (flat indices into the volume, sorted; regenerated from DUMP_SAMPLE_SEED, so two runs or two builds with the same
    arguments compare element for element)."""
    os.makedirs(out_dir, exist_ok=True)
    mid = volume.shape[1] // 2
    plane = volume[:, mid].float().cpu().numpy()
    idx = np.unique(np.random.default_rng(DUMP_SAMPLE_SEED).integers(0, volume.numel(), DUMP_SAMPLE_VOXELS, dtype=np.int64))
    sample = volume.reshape(-1)[torch.from_numpy(idx).to(volume.device)].float().cpu().numpy()
    np.save(os.path.join(out_dir, "variance_volume_plane%d.npy" % mid), np.ascontiguousarray(plane, np.float32))
    np.save(os.path.join(out_dir, "variance_volume_sample.npy"), np.ascontiguousarray(sample, np.float32))


HEADLINE_KERNEL_PREFIX = "_ZN3d3d18sweep_tiled_kernelILi1ELi4ELi16EfLb0ELi4ELi4ELi2EEE"   # sweep_tiled_kernel<1,4,16,float,false,4,4,2>


def profiled_traffic():
    """HBM bytes per launch of the dominant kernel, and what bounds it, from the committed rocprofv3 PMC profile
    (profiles/pmc_latest.json: separate FETCH_SIZE / WRITE_SIZE passes, FETCH x2 on gfx950; SQ counters in their own passes).
    Counters cannot be collected inside this process, so the numbers are reported only while the profile was taken from the SAME
    KERNEL: the profile records the SHA-256 of the kernel's gfx950 machine code in the built library (_lib.kernel_code_sha256:
    the bytes of that one function symbol -- an edit elsewhere in the source file no longer voids the profile, as round 4's file
    hash did), compared here with the library this process runs.  Returns (traffic bytes | None, info, bound fields)."""
    from deep3d_aerial_amd import _lib

    pmc = os.path.join(ROOT, "profiles", "pmc_latest.json")
    try:
        prof = json.load(open(pmc))
        sha = _lib.kernel_code_sha256(prof.get("kernel_symbol_prefix") or HEADLINE_KERNEL_PREFIX)
    except Exception:
        return None, None, {}
    ok = sha is not None and prof.get("kernel_code_sha256") == sha
    info = {"file": "profiles/pmc_latest.json", "kernel": prof.get("kernel"), "round": prof.get("round"),
            "kernel_code_sha256": prof.get("kernel_code_sha256"), "matches_loaded_library": ok}
    bound = {}
    sq, t_ns = prof.get("sq_counters_per_launch") or {}, prof.get("kernel_trace_avg_ns")
    if ok and t_ns and all(k in sq for k in ("SQ_INSTS_VALU", "SQ_LDS_IDX_ACTIVE", "GRBM_GUI_ACTIVE")):
        # what the counters say bounds the kernel: busy fractions of the vector ALUs and of the LDS pipes.
        # GRBM_GUI_ACTIVE sums the 8 XCDs' clocks; a wave64 VALU instruction occupies its SIMD for 4 cycles (16 lanes), 1024 SIMDs;
        # SQ_LDS_IDX_ACTIVE sums the busy cycles of the 256 CUs' LDS pipes.
        cycles = sq["GRBM_GUI_ACTIVE"] / 8.0
        bound = {"bound": "valu+lds", "valu_busy": round(sq["SQ_INSTS_VALU"] * 4.0 / 1024.0 / cycles, 3),
                 "lds_busy": round(sq["SQ_LDS_IDX_ACTIVE"] / 256.0 / cycles, 3), "clock_ghz": round(cycles / t_ns, 3),
                 "bound_source": "SQ_INSTS_VALU, SQ_LDS_IDX_ACTIVE, GRBM_GUI_ACTIVE of profiles/pmc_latest.json"}
    return (prof.get("hbm_bytes_per_launch") if ok else None), info, bound


def predict_strip_leg(n_views=16):
    """What a user of the reference's predict.py:126-190 loop sees: views per second of predict.predict_views
    over a 16-view strip whose neighbouring reference views share source images (predict.SyntheticStrip: 8-bit images, cropped and
    normalised on the GPU), with the by-key feature cache on and the asynchronous PFM writer putting the three products per view
    on disk -- per model, fast (h16) mode, 5 views of 2752 x 1856.  Two warm-up views pay what a process pays once (weight packing,
    graph capture); the strip itself starts with a cold feature cache and is timed whole."""
    import shutil
    import tempfile

    from deep3d_aerial_amd import predict

    out = {}
    tmp = tempfile.mkdtemp(prefix="d3d_strip_")
    try:
        strip = predict.SyntheticStrip(n_views, 5, 2752, 1856, 384, seed=3)
        items = [strip[i] for i in range(n_views)]   # decoded images + cameras: the dataset's work is not what is measured
        for name in ("casmvsnet", "adamvs", "msrednet"):
            net = predict.build_model(name, 384)
            S.fill_state_dict_(net.state_dict(), 1)
            net = net.cuda().eval()
            # one-time work stays outside: code objects loaded, weights packed (first forward of a shape) and the slice loops of the
            # recurrent models captured as HIP graphs (second forward of a shape) -- the cold feature cache is the strip's own
            predict.predict_views(net, items[:2], os.path.join(tmp, "warm"))
            torch.cuda.synchronize()
            st = {}
            t0 = time.perf_counter()
            predict.predict_views(net, items, os.path.join(tmp, name), feature_cache_bytes=32 << 30, stats=st)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            files = len(os.listdir(os.path.join(tmp, name)))
            out[name] = {"views_per_s": round(n_views / dt, 2), "ms_per_view": round(dt / n_views * 1e3, 2), "files_written": files,
                         "pyramids_per_view": round(st.get("pyramids_per_view", 0.0), 2),
                         "cache_hit_rate": round(st.get("cache_hits", 0) / max(1, st.get("cache_hits", 0) + st.get("cache_misses", 0)), 3)}
            del net
            torch.cuda.empty_cache()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    out["workload"] = "%d-view strip, 5 views of 2752 x 1856 per reference view, feature cache + asynchronous PFM writer on, h16 mode" % n_views
    return out


def _lib_h16():
    from deep3d_aerial_amd import _lib

    return _lib.h16_format()


def secondary_models(reps=5, warm=2):
    """BASELINE config 3 (not the headline metric): one reference view of the full cascades at 2752x1856, 5 views, bf16
    regulariser operands, seeded random weights -- ms per view and cost-volume Mvoxels/s (97.05 M voxels per view)."""
    from deep3d_aerial_amd import predict

    res = {}
    old = ops.conv_precision()
    ops.set_conv_precision("h16")
    try:
        for name in ("casmvsnet", "adamvs", "msrednet"):
            net = predict.build_model(name, 384)
            S.fill_state_dict_(net.state_dict(), 1)
            net = net.cuda().eval()
            s = predict.SyntheticBlock(1, 5, 2752, 1856, 384)[0]
            imgs = torch.from_numpy(s["imgs"])[None].cuda()
            pm = {k: torch.from_numpy(v)[None].cuda() for k, v in s["proj_matrices"].items()}
            dv = torch.from_numpy(s["depth_values"])[None].cuda()
            ops.note_depth_range(dv, s["depth_values"][0], s["depth_values"][-1])   # as predict.predict_views hands it over: no host sync per view
            with torch.no_grad():
                for _ in range(warm):   # (the first forward packs the weights; the second settles the allocator's pools)
                    net(imgs, pm, dv)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    net(imgs, pm, dv)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) / reps * 1e3
            res[name] = {"ms_per_view": round(ms, 2), "mvoxels_per_s": round(97.05e6 / ms / 1e3, 1)}
            # which kernels served the view (ops.dispatch_counts; the sweeps' families come from the C dispatcher's own counters)
            ops.dispatch_counts.clear()
            ops.sweep_dispatch_counts(reset=True)
            with torch.no_grad():
                net(imgs, pm, dv)
            torch.cuda.synchronize()
            res[name]["dispatch"] = {**dict(ops.dispatch_counts), "sweeps": ops.sweep_dispatch_counts()}
            del net, imgs, pm, dv
            torch.cuda.empty_cache()
        res["predict_strip"] = predict_strip_leg()
        res["casmvsnet"]["regulariser"] = regulariser_leg()
        res["cascade_sweeps"] = cascade_sweeps_leg()
    finally:
        ops.set_conv_precision(old)
    res["config"] = "config 3: full cascade forward, 5 views, 2752x1856, ndepths 48/32/8, 16-bit regulariser operands in the library's h16 format (%s; fp32 accumulate), synthetic" % _lib_h16()
    return res


def cascade_sweeps_leg(reps=5):
    """The cost-volume sweeps of a cascade view on their own: the three stage shapes of config 3
    (5 views; stage 1 per-plane depths, stages 2 / 3 per-pixel hypotheses as (lo, step) maps, as cas_mvsnet.py passes them),
    planar fp32 variance, visibility-weighted correlation and the channel-last bf16 variance volume of the bf16 regulariser:
    ms per launch and the fraction of 8 TB/s on the algorithmic bytes (source maps + hypothesis maps read once, volume
    written once).  Scene and shapes are tools/stage_sweep_bench.py's."""
    H, W = 1856, 2752
    out = {}
    for tag, C, D, sc, perpix in (("stage1", 32, 48, 4, False), ("stage2", 16, 32, 2, True), ("stage3", 8, 8, 1, True)):
        h, w = H // sc, W // sc
        proj, dv = S.make_scene(5, h, w, 384 // (1 if not perpix else 4), seed=3)
        feats = [torch.randn(C, h, w, device="cuda") for _ in range(5)]
        p34 = ops.compose_projections(torch.from_numpy(proj).cuda())
        if perpix:
            base = torch.full((h, w), float(dv.mean()), device="cuda")
            depth = ops.depth_range_affine(base, D, float(dv[1] - dv[0]) / 384 * sc)
        else:
            depth = torch.from_numpy(S.uniform_depths(dv, D)).cuda()
        vw = torch.rand(4, h, w, device="cuda")
        reads = 5 * C * h * w * 4 + (2 * h * w * 4 if perpix else 0)

        def timed(fn):
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / reps

        t_var = timed(lambda: ops.variance_volume(feats, p34, depth))
        t_w = timed(lambda: ops.weighted_corr(feats, p34, vw, depth))
        t_cl = timed(lambda: ops.variance_volume_cl(feats, p34, depth, layout="cl8"))
        out[tag] = {"shape": "C %d x D %d x %d x %d" % (C, D, h, w),
                    "variance_ms": round(t_var, 3), "variance_hbm_frac": round((reads + C * D * h * w * 4) / t_var / 8e9, 3),
                    "weighted_ms": round(t_w, 3),
                    "variance_cl_bf16_ms": round(t_cl, 3), "variance_cl_bf16_hbm_frac": round((reads + C * D * h * w * 2) / t_cl / 8e9, 3)}
        del feats, depth, vw
        torch.cuda.empty_cache()
    return out


def regulariser_leg(reps=5):
    """The three CostRegNets of a CasMVSNet view alone (bf16 mode, channel-last bf16 activations, the volume as the sweep
    kernel leaves it): ms, algorithmic HBM bytes (every layer reads its input and skip once and writes its output once, in
    the formats they travel in) against 8 TB/s, and the 3-D convolution FLOPs against the 2.5 PFLOP/s dense bf16 peak."""
    from deep3d_aerial_amd.cas_mvsnet import CostRegNet

    total_ms, total_bytes, total_flop = 0.0, 0.0, 0.0
    for C, D, h, w in ((32, 48, 464, 688), (16, 32, 928, 1376), (8, 8, 1856, 2752)):
        net = CostRegNet(C).cuda().eval()
        S.fill_state_dict_(net.state_dict(), 3)
        vol = ops.cl_to_cl8(torch.randn(D, h, w, C, device="cuda").to(ops.h16_dtype()))   # [D,C/8,h,w,8]: as the sweep kernels write it
        with torch.no_grad():
            net.forward_one(vol)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                net.forward_one(vol)
            e1.record()
            torch.cuda.synchronize()
        total_ms += e0.elapsed_time(e1) / reps
        v = D * h * w
        # (C_in, C_out, input voxels, output voxels, skip): conv0..conv6, conv7/9/11 (transposed, with skip), prob
        layers = [(C, 8, v, v, 0), (8, 16, v, v // 8, 0), (16, 16, v // 8, v // 8, 0), (16, 32, v // 8, v // 64, 0),
                  (32, 32, v // 64, v // 64, 0), (32, 64, v // 64, v // 512, 0), (64, 64, v // 512, v // 512, 0),
                  (64, 32, v // 512, v // 64, 1), (32, 16, v // 64, v // 8, 1), (16, 8, v // 8, v, 1)]
        for ci, co, vi, vo, sk in layers:
            total_bytes += 2.0 * ci * vi + 2.0 * co * vo * (1 + sk)
            total_flop += 2.0 * 27 * ci * co * (vo if vo <= vi else vi)   # a transposed layer does 27 MACs per INPUT voxel and channel pair
        total_bytes += 2.0 * 8 * v + 4.0 * v            # prob: channel-last in, fp32 plane out
        total_flop += 2.0 * 27 * 8 * v
        del net, vol
        torch.cuda.empty_cache()
    return {"ms": round(total_ms, 2), "algorithmic_bytes": int(total_bytes), "gbps": round(total_bytes / total_ms / 1e6, 1),
            "hbm_frac": round(total_bytes / total_ms / 1e6 / 8000.0, 3), "flop": total_flop,
            "tflops": round(total_flop / total_ms / 1e9, 1), "mfma_frac": round(total_flop / total_ms / 1e9 / 2500.0, 4),
            "formats": "channel-last 16-bit activations (%s), fp32 probability volume out" % _lib_h16()}


def exchange_leg(dist, rank, world, shared, reps=3):
    """BASELINE config 5's one collective, outside the timed region: the all-gather of the ranks' (depth, confidence) maps ahead
    of fusion (sharding.all_gather_maps -> pipeline.predict_and_fuse), at config 5's map size 3712 x 2752 fp32.  One process per
    GPU: 8 reference views per rank (64 views over 8 GPUs) through RCCL; ranks sharing a card (a rehearsal, gloo through host
    memory): 1 view per rank.  Median of `reps`, barrier + synchronize on both sides, MAX over ranks."""
    from deep3d_aerial_amd import sharding

    n_local = 1 if shared else 8
    h, w = 3712, 2752
    local = torch.full((n_local, 2, h, w), float(rank), dtype=torch.float32, device="cuda")
    times = []
    for _ in range(reps + 1):
        dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        full = sharding.all_gather_maps(local, n_local * world, rank, world)
        torch.cuda.synchronize()
        dist.barrier()
        times.append(time.perf_counter() - t0)
    ok = bool(all(float(full[r * n_local, 0, 0, 0]) == r for r in range(world)))
    t = torch.tensor([sorted(times[1:])[len(times[1:]) // 2]], dtype=torch.float64, device="cpu" if shared else "cuda")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    ms = float(t.item()) * 1e3
    per_rank_bytes = n_local * 2 * h * w * 4
    return {"allgather_ms": round(ms, 3), "shape_per_rank": [n_local, 2, h, w], "dtype": "f32", "bytes_per_rank": per_rank_bytes,
            "bytes_gathered": per_rank_bytes * world, "backend": dist.get_backend(),
            "gbps_per_rank_in": round(per_rank_bytes * (world - 1) / (ms * 1e-3) / 1e9, 1), "content_ok": ok,
            "what": "config 5: all-gather of the depth / confidence maps ahead of fuse/consistency_check_n.py"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run the parity check, the CPU baselines and the config-3 model timings "
                         "(N = 1) or the config-5 exchange (N > 1), and add them to the line")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines and the parity check")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip the config-3 model timings")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step computed to DIR/*.npy (rank 0; see dump_outputs)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world != args.gpus:
        sys.exit("launch with torch.distributed.run --nproc-per-node %d (WORLD_SIZE=%d)" % (args.gpus, world))
    ndev = torch.cuda.device_count()
    # one process per GPU; with fewer devices than ranks (a rehearsal of the N > 1 path on a one-GPU box) the ranks share
    # the card and the two control-plane collectives below go through gloo on host tensors
    shared = world > 1 and ndev < world
    if shared and os.environ.get("D3D_BENCH_SHARE_GPU", "0") != "1":
        # a scaling run must have one device per rank: sharing a card is a rehearsal of the control path only, and has to be
        # asked for (tests/test_sharding_gpu.py does), never fallen into
        sys.exit("bench.py --gpus %d: %d ranks but only %d visible device(s); set D3D_BENCH_SHARE_GPU=1 to rehearse the "
                 "N > 1 path with ranks sharing a card" % (args.gpus, world, ndev))
    torch.cuda.set_device(local_rank % max(ndev, 1))
    dist = None
    if world > 1:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo" if shared else "nccl", rank=rank, world_size=world)

    # every rank builds its own reference view (seed = rank): independent work items
    proj, dv = S.make_scene(V, H_FEAT, W_FEAT, D, seed=rank)
    feats_host = S.make_features(V, C, H_FEAT, W_FEAT, seed=rank)
    depth_host = S.uniform_depths(dv, D)
    in_frame = S.in_frame_fraction(proj, depth_host, H_FEAT, W_FEAT)
    feats = [torch.from_numpy(f).cuda() for f in feats_host]
    depth = torch.from_numpy(depth_host).cuda()
    p34 = ops.compose_projections(torch.from_numpy(proj).cuda())
    out = torch.empty((C, D, H_FEAT, W_FEAT), dtype=torch.float32, device="cuda")

    def step():
        ops.variance_volume(feats, p34, depth, out=out)

    for _ in range(args.warmup):
        step()
    starts = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps)]
    stops = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps)]

    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        starts[i].record()  # same stream as the kernel (torch's current stream is passed to the C ABI)
        step()
        stops[i].record()
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    local_elapsed = elapsed
    if dist:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if shared else "cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    kern_ms = float(np.mean([s.elapsed_time(e) for s, e in zip(starts, stops)]))
    per_rank = None
    if dist:
        # what a first multi-GPU run needs to be diagnosable: every rank's own kernel time, wall time and device
        mine = {"rank": rank, "kernel_ms": round(kern_ms, 4), "elapsed_s": round(local_elapsed, 5),
                "device_index": local_rank % max(ndev, 1), "device": torch.cuda.get_device_name(),
                "in_frame_fraction": round(in_frame, 4)}
        per_rank = [None] * world
        dist.all_gather_object(per_rank, mine)
    exchange = None
    if dist and args.full:
        try:
            exchange = exchange_leg(dist, rank, world, shared)
        except Exception as e:   # the scaling line must survive a failure of the add-on leg (reported, not hidden)
            exchange = {"error": repr(e)[:300]}
    voxels = D * H_FEAT * W_FEAT
    value = world * args.steps * voxels / elapsed / 1e6
    achieved = algorithmic_bytes() / (kern_ms * 1e-3) / 1e9

    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, out)   # outside every timed region; `out` holds the last timed step's volume

    if rank == 0:
        traffic, traffic_info, bound = profiled_traffic()
        line = {
            "metric": "cost-volume Mvoxels/s (5v x 384D)",
            "value": round(value, 1),
            "unit": "Mvoxels/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {"workload": "config 2: fused homography-warp + variance, 5 views x 384 planes, "
                                   "features 32x688x464 fp32 (2752x1856 image at 1/4 res), one reference view per "
                                   "step per GPU", "voxels_per_step_per_gpu": voxels,
                       "in_frame_fraction": round(in_frame, 4), "path": (config.switches.get("D3D_FORCE_PATH") or "auto"),
                       **({"ranks_share_one_gpu": True} if shared else {})},
            # achieved / peak / frac price the kernel against the HBM roofline (its algorithmic bytes) -- the bar the
            # north star sets; `bound` says what the counters show it is actually limited by (vector ALU + LDS issue)
            "roofline": {"bound": bound.get("bound", "valu+lds"), "priced_against": "hbm", "achieved": round(achieved, 1),
                         "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic,
                         **{k: v for k, v in bound.items() if k != "bound"}, "traffic_profile": traffic_info,
                         "kernel_ms": round(kern_ms, 4), "algorithmic_bytes": algorithmic_bytes(),
                         **issue_floor_fields(kern_ms)},
        }
        if per_rank is not None:
            line["per_rank"] = per_rank
        if exchange is not None:
            line["exchange"] = exchange
        if world == 1 and args.full and not args.no_cpu_baseline:
            p34_host = p34.cpu().numpy().reshape(-1, 3, 4)
            cb, parity = cpu_baseline(p34_host, feats_host, depth_host, gpu_volume=out)
            line["parity"] = parity
            # second baseline of SURVEY.md 8(d): the reference's op sequence in plain PyTorch CPU, all cores and 8 threads
            allc = host_threads()
            cb["torch_ops_all_cores"] = torch_cpu_leg(proj, feats_host, depth_host, allc)
            cb["torch_ops_8_threads"] = torch_cpu_leg(proj, feats_host, depth_host, min(8, allc))
            line["cpu_baseline"] = cb
        if world == 1 and args.full and not args.no_secondary:
            del out
            torch.cuda.empty_cache()
            try:
                line["secondary"] = secondary_models()
            except Exception as e:   # the headline line must survive a failure of the add-on
                line["secondary"] = {"error": repr(e)[:200]}
        print(json.dumps(line), flush=True)
    if dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
