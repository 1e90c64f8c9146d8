// LDS-tiled plane-sweep kernel for gfx950 (MI355X): the fast path behind d3d_variance_volume,
// d3d_weighted_corr, d3d_pair_corr_mean and d3d_homo_warp.
//
// Why a tiled kernel: per voxel and source view a bilinear sample touches 4 taps x C channels
// (2 KB per voxel at C = 32, V = 5) while only 4*C bytes are written, so the gather must not
// go to L2 -- it is served from LDS.  Design (numbers in DESIGN.md):
//
//   * One workgroup (8 compute + 4 loader waves) = a 32 x 4 patch of reference pixels x a segment
//     of depth planes x a group of CH channels.  It walks the segment in STEPS of SP = NSUB*m
//     planes: compute wave (pw, sub) owns two patch rows and the planes d = step*SP + sub + NSUB*j.
//     A last patch column with at most 16 real pixels per row is swept in 16 x 8 patches instead (half as many workgroups
//     there, none of them half empty): same lanes, same loop, another lane -> pixel map.
//   * The source footprint of (patch x step) is bounded per view by projecting the 8 corners of
//     the frustum slab (valid because the map is projective and p.z > 0 at every corner).  All
//     step windows of the segment are planned ONCE in the prologue, one lane per step.
//   * Each view owns a RING in LDS: a torus of RW x RH positions, channel-last
//     ([position][CH+4 floats]; the +4 pad spreads ds_read_b128 over all 64 banks), with column
//     RW and row RH duplicating column 0 and row 0 so that the east/south taps never wrap.
//     Moving to the next step only stages the thin L-shaped difference of consecutive windows.
//     RW/RH are at least the span of the UNION of any two consecutive windows, so the slots
//     that difference lands in are never part of the window being read: the loader waves
//     write step k+1's difference while the compute waves work on step k, and one barrier per
//     step is the only synchronisation.  Compute waves never wait on a global load.  Positions
//     outside the source image are staged as zeros (= per-tap zero padding).
//   * Compute: a lane owns one reference pixel and CH channels.  Per plane it does the geometry
//     ONCE per view (3 mul/add, rcp + Newton, floor/fract, window test, ring address) and then,
//     per channel quad and view, four ds_read_b128 feed 4 x (4 interpolation + 2 accumulation)
//     VALU ops; the reads of the next (quad, view) unit are issued before the current one is
//     blended.  Lanes are permuted so that each hardware ds_read_b128 lane group covers 16
//     consecutive pixels (conflict-free for unit-scale sweeps).  Results leave as 128-byte row
//     segments per (channel, plane) -- full-line HBM writes -- through scalar-base stores.
//   * If the rings cannot be made to fit (p.z <= 0 at a corner, extreme scale/rotation) the
//     workgroup runs the same loop nest with taps gathered from global memory instead.
//
// Nothing is reshaped into a GEMM: this is HBM-write-bound streaming work with an LDS-fed
// gather, not MFMA work.
#include "common.h"

#include <hip/hip_fp16.h>

#include "sweep_params.h"
#include "sweep_device.h"

#include <cstdlib>

namespace d3d {

namespace {

constexpr int TW = 32;          // patch width  (one 128-byte output row segment per lane-row)
// The wave counts of a workgroup are template parameters of the kernel (NSUB, NLOADW, NPIXW; the patch is 2 * NPIXW rows high).
// These are the DEFAULT workgroup's, read by the host code only: 2 x 4 compute + 4 loader waves = 12 waves, 3 per SIMD at the
// 168-VGPR budget, sweeping a 32 x 4 patch.  (launch_one picks SHALLOW_* instead for shallow sweeps.)
#ifndef D3D_NSUB
#define D3D_NSUB 4
#endif
#ifndef D3D_NLOADW
#define D3D_NLOADW 4
#endif
constexpr int DEFAULT_NSUB = D3D_NSUB;      // depth sub-ranges
constexpr int DEFAULT_NLOADW = D3D_NLOADW;  // loader waves: stage the next step's window delta into the rings (0: the compute waves do)
constexpr int DEFAULT_NPIXW = 2;            // pixel waves (2 patch rows each)
constexpr int DSEG_MAX = 128;   // planes per workgroup segment upper bound (launch_one never asks for more)
constexpr int MAXSTEPS = 64;    // >= DSEG_MAX / NSUB for every NSUB launched, <= 64 (one lane per step)
constexpr int PFD = 2;          // delta staging items (64 positions x CH channels) a loader wave keeps in flight
constexpr int LDS_PIPE = 1;     // (quad, view) units whose taps are requested ahead of the one being blended
constexpr int NCAND = 4;        // candidate step sizes: 4, 2, 1, 1/2 times NSUB planes
constexpr int MAXRECTS = 512;   // non-empty delta rectangles per workgroup segment (4 words each)
// LDS bank layout of the rings (tools/bank_sim.py models it on config 2; PMC: SQ_LDS_BANK_CONFLICT).  A ds_read_b128 is
// serviced in four 16-lane groups, one 16-byte slot (4 banks) per lane, 16 slots per LDS cycle.  A lane group holds an
// 8 x 2 block of reference pixels (lane -> pixel map below), whose taps span < 8 columns and 2 (rarely 3) rows of a
// source view for scales up to 1.14.  With a position stride of an ODD number of slots (STRIDE = CH + 4 floats) and a
// row pitch of 8 slots mod 16 (32 floats mod 64), two positions share a slot only if they lie (16,0), (8,1) or (0,2)
// apart -- outside such a block.  The torus wrap keeps that property when RW is a multiple of 8 and RH is even.
// Round 1 (16 x 1 pixels per group, unpadded pitch): 6.2 LDS cycles per tap read on config 2; this layout: 4.3.
constexpr int RING_RW_QUANT = 8;
constexpr int RING_RH_QUANT = 2;
template <int STRIDE>
__host__ __device__ __forceinline__ int ring_row_floats(int RW) {
    const int n = (RW + 1) * STRIDE;
    return ((n - 32 + 63) & ~63) + 32;   // smallest pitch >= n that is 32 mod 64
}

// Cycle stamps and plan statistics of the kernel (D3D_TILED_STATS): compiled only into -DD3D_EXPERIMENTS builds -- in the
// production kernel the stamps and their accumulators would be live scalar registers across the plane loop.
#ifdef D3D_EXPERIMENTS
#define D3D_STAMPS 1
#else
#define D3D_STAMPS 0
#endif
#define D3D_CLOCK() (D3D_STAMPS ? clock64() : 0ll)

struct TiledArgs {
    int ngroups;     // channel groups (C / CH), one workgroup pass each
    int dseg;        // planes per workgroup segment
    int cap_floats;  // floats available for the rings
    int nseg;        // segments along depth
    int tiles_x, tiles_y;
    int tall;        // 1: the last patch column holds at most TW/2 real pixels per row and is swept in TALL patches (see the block decode)
    const float* cl;  // channel-last copy of the source maps [view][group][h*w][CH] (pack_channel_last_kernel), or null
    unsigned long long* tstats;  // debug timing (cycles, wave 0): [0] prologue [1] barrierA+write+barrierB [2] issue [3] compute [4] total
    unsigned* stats;  // debug (D3D_TILED_STATS): [0] ring wgs [1] fallback wgs [2] sum m [3] sum nsteps [4] sum ring floats [5] staging items [6] of them inside one rectangle [7] plain (kind 0) [8] of [6] inside the image [9] of [6] clear of ring column 0 and row 0 [10] slots of a staging round with no item left
};

// LDS map (ints/floats):
//   [zero cell 2*STRIDE][pmin DSEG_MAX][pmax DSEG_MAX][header 32][view constants 8*NSRC]
//   [plan table MAXSTEPS*NSRC*8][rect starts MAXSTEPS+4][positions per step MAXSTEPS][rect descriptors (MAXRECTS+1)*4][rings ...]
// header: 0 mode (1 rings, 0 global gather) | 1 planes per step | 2 nsteps | 4+4i.. RW, RH, base, RW | RH << 8 | (base/4) << 16 per view
// plan entry (per step, view): wx0, wy0, ww, wh, ox, oy, ox - wx0, oy - wy0
// rect descriptor (non-empty delta rectangles, grouped by step), 4 words:
//   (rx + 1) | (ry + 1) << 16,  width | view << 12 | first position (cumulative within the step) << 16,
//   positions,  ring col | row << 16 of the rect origin (unwrapped)
template <int CW, int NSRC>   // CW = 4-byte words per ring position (CH fp32 channels, or CH/2 words of fp16 pairs)
struct Lds {
    static constexpr int STRIDE = CW + 4;
    static constexpr int ZERO = 0;
    static constexpr int PMIN = 2 * STRIDE;
    static constexpr int PMAX = PMIN + DSEG_MAX;
    static constexpr int HDR = PMAX + DSEG_MAX;
    static constexpr int VT = HDR + 32;                // per view: T0, T1, T2, -, RW, RH, row bytes, absolute ring base (view-major plane loop)
    static constexpr int PLAN = VT + 8 * NSRC;
    static constexpr int SST = PLAN + MAXSTEPS * NSRC * 8;
    static constexpr int STOT = SST + MAXSTEPS + 4;   // positions to stage per step
    static constexpr int RECTS = ((STOT + MAXSTEPS + 3) / 4) * 4;
    static constexpr int DATA = RECTS + (MAXRECTS + 1) * 4;  // 16-byte aligned
};

__device__ __forceinline__ int posmod(int a, int n) {
    int r = a % n;
    return r < 0 ? r + n : r;
}


// Wave-uniform constants of one source view's ring (scalar registers in the plane loop).
struct RingView {
    int RW, RH;  // torus size in positions
    int rowb;    // bytes between ring rows
    int base;    // absolute LDS byte address of ring position (0, 0)
};

// Projection + bilinear weights + ring addresses of one (pixel, plane, view): ~34 VALU instructions, no branches, no
// predicates.  (u, v) are CLAMPED to [-1, w] x [-1, h] instead of being tested against the window: the planner clamps the
// hull of the patch the same way (monotone, so a clamped sample lies in the clamped hull), windows may reach one position
// past the image on the left / top and two on the right / bottom, and every position outside the image is staged as
// zeros -- a sample outside the image reads zero taps (or taps of weight exactly 0), which is per-tap zero padding.
// (kx, ky) = ring offset minus window origin of the current step.  Non-finite projections end at a clamp bound
// (v_med3_f32 returns the smallest operand when one is a NaN).
template <int STRIDE>
__device__ __forceinline__ TapL geo_ring(const Ray& r, float tx, float ty, float tz, float d, float umax, float vmax, int kx, int ky,
                                         const RingView& R) {
    const float px = __fadd_rn(__fmul_rn(r.rx, d), tx);
    const float py = __fadd_rn(__fmul_rn(r.ry, d), ty);
    const float pz = __fadd_rn(__fmul_rn(r.rz, d), tz);
    // quotient = v_rcp_f32 estimate + one Newton correction (correctly rounded in practice: common.h project())
    const float iz = __builtin_amdgcn_rcpf(pz);
    const float u0 = px * iz, v0 = py * iz;
    float u = fmaf(fmaf(-u0, pz, px), iz, u0);
    float v = fmaf(fmaf(-v0, pz, py), iz, v0);
    u = __builtin_amdgcn_fmed3f(u, -1.0f, umax);
    v = __builtin_amdgcn_fmed3f(v, -1.0f, vmax);
    const float fu = floorf(u), fv = floorf(v);
    const float ax = u - fu, ay = v - fv;
    const float bx = (fu + 1.0f) - u, by = (fv + 1.0f) - v;
    TapL t;
    t.nw = bx * by;
    t.ne = ax * by;
    t.sw = bx * ay;
    t.se = ax * ay;
    unsigned c = (unsigned)((int)fu + kx), rr = (unsigned)((int)fv + ky);
    c = min(c, c - (unsigned)R.RW);  // one conditional wrap: 0 <= c < 2 RW
    rr = min(rr, rr - (unsigned)R.RH);
    t.a0 = R.base + (int)__umul24(rr, (unsigned)R.rowb) + (int)__umul24(c, (unsigned)(STRIDE * 4));
    t.a1 = t.a0 + R.rowb;
    return t;
}


// fp16 storage: one 2-byte store per lane (a wave writes two 64-byte row segments per channel and plane)
__device__ __forceinline__ void store_sbase_h(unsigned long long sb, unsigned byte_off, float v) {
    const _Float16 hv = (_Float16)sat_f16(v);   // RNE, saturating like every h16 data store (common.h)
    const unsigned bits = __builtin_bit_cast(unsigned short, hv);
    asm volatile("global_store_short %0, %1, %2 nt" : : "v"(byte_off), "v"(bits), "s"(sb));
}
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
// fp32 fma whose first factor is the LOW / HIGH fp16 half of a 32-bit word (v_fma_mix_f32): the fp16 tap is widened
// inside the instruction -- exact -- so no conversion instruction and no fp32 copy of the tap exist (hipcc prefers
// v_cvt_f32_f16 + packed fp32 fma here: 32 more instructions and 32 more live registers per 8-channel unit).
__device__ __forceinline__ float fma_mix_lo(float pair, float w, float acc) {
    float d;
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(d) : "v"(pair), "v"(w), "v"(acc));
    return d;
}
__device__ __forceinline__ float fma_mix_hi(float pair, float w, float acc) {
    float d;
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(pair), "v"(w), "v"(acc));
    return d;
}
__device__ __forceinline__ float ldf(const float* q) { return *q; }
__device__ __forceinline__ float ldf(const __half* q) { return __half2float(*q); }

}  // namespace

// T = float: tensors as declared in SweepParams.  T = __half (MODE_VARIANCE only; BASELINE config 5): feats[] and out
// are fp16 tensors of the same shapes, the rings hold fp16 cells (half the LDS bytes per tap), every product and sum
// is fp32 (v_fma_mix_f32 reads the fp16 tap directly), the result is rounded once (RNE) at the store.
// OUTCL: the variance volume leaves as a channel-last bf16 volume [D][h][w][C] (RNE) -- the form conv0 of the 3-D
// regulariser stages in bf16 mode (conv_c8.hip); four channels of a voxel = one 8-byte store instead of four 4-byte ones.
// NSUB / NLOADW: depth sub-ranges and loader waves of a workgroup.  The default (4 + 4: 12 waves, all of a CU's LDS) is
// sized for deep sweeps; SHALLOW sweeps (the last cascade stage: 8 planes) run 2 + 2 = 6 waves on half the LDS, so TWO
// workgroups share a CU and one's planning prologue and first-window latency (most of its life: 47 % + 40 % at 8 planes)
// overlap the other's arithmetic.
template <int MODE, int NSRC, int CH, typename T = float, bool OUTCL = false, int NSUB = D3D_NSUB, int NLOADW = D3D_NLOADW,
          int NPIXW = 2>
__global__ __launch_bounds__(64 * (NPIXW * NSUB + NLOADW), 3) void sweep_tiled_kernel(SweepParams p, TiledArgs a) {   // 3 waves per SIMD: the 168-register budget for either workgroup size
    constexpr int TH = 2 * NPIXW;   // patch height
    constexpr int NCOMP = NPIXW * NSUB, NWAVES = NCOMP + NLOADW, THREADS = 64 * NWAVES;   // compute waves | all waves
    constexpr bool F16 = sizeof(T) == 2;
    static_assert(!OUTCL || (MODE == MODE_VARIANCE && !F16), "channel-last bf16 output is built for the fp32 variance volume");
    constexpr int CW = CH * (int)sizeof(T) / 4;   // words per ring position
    constexpr int CPC = 16 / (int)sizeof(T);      // channels per 16-byte chunk (one ds_read_b128): 4 | 8
    using L = Lds<CW, NSRC>;
    constexpr int STRIDE = L::STRIDE;
    constexpr int Q = CW / 4;                     // 16-byte chunks per position
    static_assert(!F16 || MODE == MODE_VARIANCE, "fp16 storage is built for the variance volume only");
    constexpr bool VIEW_MAJOR = F16;             // unit order of the compute loop (see there)
    constexpr int MAXRS = 4 * NSRC;               // delta rectangles a step can have (left | right | top | bottom per view)
    static_assert(NSRC <= 7, "rect descriptors keep the view in 4 bits; the planner scans 5-bit rectangle counts");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int* ldsi = reinterpret_cast<int*>(lds);

    const long long t_start = D3D_CLOCK();
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = rfl(tid >> 6);
    const bool loader = wave >= NCOMP;
    const int lw = wave - NCOMP;                 // loader index
    const int pw = (wave % NCOMP) % NPIXW;       // which pair of patch rows
    const int sub = (wave % NCOMP) / NPIXW;      // depth sub-range
    const int h = p.h, w = p.w, D = p.D;
    const size_t plane = (size_t)h * w;

    // block -> (patch row, segment, channel group, patch column).  Blocks b, b+8, ... share an XCD
    // (and its L2): give each XCD a contiguous run of the logical order.
    int b = blockIdx.x;
    {
        const int nblk = gridDim.x;
        const int per = nblk / 8;
        // (Only when the XCDs get equal runs.  Ragged runs for every block count -- x * per + min(x, nblk % 8) -- were measured on
        //  config 2, 7482 workgroups: the sweep fetches 3.3 times less from HBM and takes 5 % longer, profiles/loader_decode_ab.txt.)
        if (nblk % 8 == 0) b = (b % 8) * per + b / 8;
    }
    // Within an XCD's run, vertically adjacent patches come first: they share most of their source
    // rows (same depth segment, same channel group), so the windows of the ~32 workgroups an XCD runs
    // concurrently overlap in its L2 instead of each being fetched from HBM.
    // TALL patches: when the last patch column holds at most TW/2 real pixels per row (a.tall; 464 = 14 * 32 + 16), a TW-wide
    // patch there would issue every instruction of the plane loop for half a patch of EXEC-masked lanes.  Two vertically
    // adjacent half-empty patches are folded into one patch of TW/2 x 2 TH pixels instead: the column takes ceil(tiles_y / 2)
    // workgroups per segment, which follow the wide columns in the logical order (vertically adjacent ones still adjacent).
    // `tall` is wave-uniform and only read here and by the planner: the plane loop sees nothing but its lanes' pixels.
    const int nwide = a.tall ? (a.tiles_x - 1) * a.tiles_y * a.nseg : 0x7fffffff;
    const bool tall = b >= nwide;
    if (tall) b -= nwide;
    const int tyn = tall ? (a.tiles_y + 1) >> 1 : a.tiles_y;   // patches per column
    const int PW = tall ? TW / 2 : TW, PH = tall ? 2 * TH : TH;   // this workgroup's patch rectangle
    const int pwsh = tall ? 4 : 5;   // log2(PW)
    const int ty = b % tyn;
    const int seg = (b / tyn) % a.nseg;
    const int tx = tall ? a.tiles_x - 1 : b / (tyn * a.nseg);
    // The workgroup sweeps ALL channel groups of its (patch, depth segment), one after the other: the plan (windows,
    // step size, staging rectangles) does not depend on the channels, so the prologue is paid once.
    const int x0 = tx * TW, y0 = ty * PH;
    const int ds = seg * a.dseg;
    const int de = min(ds + a.dseg, D);
    const int nplanes = de - ds;
    const int x1c = min(x0 + PW - 1, w - 1), y1c = min(y0 + PH - 1, h - 1);

    // Lane -> pixel.  ds_read_b128 is serviced in the lane groups {0-3,12-15,20-27} and
    // {4-11,16-19,28-31} (+32; confirmed with tools/lds_groups.hip): each group takes an 8 x 2 block of
    // pixels (bank layout: see ring_row_floats).  Lanes 0-15 / 16-31 / 32-47 / 48-63 each hold 16
    // consecutive pixels of one row, so a store instruction still writes whole 64-byte row segments.
    // Lanes 32-63 repeat the 16 x 2 block of lanes 0-31 sixteen columns to the right -- in a tall patch TH rows further
    // down: a pixel wave then owns the rows {2 pw, 2 pw + 1} and {2 pw + TH, 2 pw + TH + 1}, 16 pixels each.
    const int l5 = lane & 31;
    const int pxl = (l5 < 4) ? l5 : (l5 < 12) ? l5 + 4 : (l5 < 20) ? l5 - 8 : (l5 < 28) ? l5 - 20 : l5 - 16;
    const int px = x0 + pxl + (tall ? 0 : 16 * (lane >> 5));
    const int py = y0 + pw * 2 + (l5 >> 4) + (tall ? TH * (lane >> 5) : 0);
    const bool valid = (px < w) && (py < h);
    const int pix = valid ? py * w + px : 0;
    const unsigned pixb = (unsigned)pix * (unsigned)sizeof(T);  // per-lane byte offset (h*w < 2^30)
    // channel-last cells: C * 2 bytes per pixel (h*w*C*2 < 2^32, checked at launch), or 16 in a plane of 8-channel groups (CL8)
    const unsigned pixo = OUTCL ? (p.out_cl == 2 ? (unsigned)pix * 16u : (unsigned)pix * (unsigned)p.C * 2u) : pixb;
    const float xf = (float)px, yf = (float)py;

    // --- per-lane inputs of the compute waves, requested BEFORE the planning phases below so that their global-memory latency
    //     (projection rows, the reference features of the first channel group, view weights, hypothesis maps) runs under
    //     the planning instead of after it: on the cascade's shallow sweeps the prologue is most of a workgroup's life ----
    //     (Up to four source views.  With six, 36 more registers live across the planning make the plane loop spill.)
    constexpr bool EARLY_INPUTS = NSRC <= 4 && !F16 && CH <= 16;
    // Per-plane depths are requested FIRST: loads return in order, so a wait for a load issued behind the per-lane inputs would
    // be a wait for all of them (the reference features come from HBM), and the first barrier of the planning waits for this one.
    // The LOADER waves fetch them (one thread per plane): they request no per-lane inputs, so the wait the compiler places in front
    // of the LDS write -- for every load of whichever wave gets there -- is a wait for this load alone.
    constexpr bool DEPTH_BY_LOADERS = NLOADW * 64 >= DSEG_MAX;
    static_assert(THREADS >= DSEG_MAX, "one thread per plane of a segment");
    const int dtid = DEPTH_BY_LOADERS ? tid - 64 * NCOMP : tid;
    float dplane = 0.0f;
    if (p.depth_mode == D3D_DEPTH_PER_PLANE && dtid >= 0 && dtid < nplanes) dplane = p.depth[ds + dtid];
    // ... and the projection rows of the view this wave plans (wave i: view i), which the planner reads after that barrier
    float mw[12];
    {
        const float* __restrict__ Mg = p.proj34 + 12 * min(min(wave, NSRC - 1), p.n_src - 1);
#pragma unroll
        for (int k = 0; k < 12; ++k) mw[k] = Mg[k];
    }
    int grp = 0, c0 = 0;  // current channel group / its first channel
    Ray ray[NSRC];
    float T0[NSRC], T1[NSRC], T2[NSRC];
    auto projection_rows = [&]() {
        // (every view's rows are requested before the first of them is used: one latency instead of one per view)
        float m[NSRC][12];
#pragma unroll
        for (int i = 0; i < NSRC; ++i) {
            const float* __restrict__ Mg = p.proj34 + 12 * min(i, p.n_src - 1);
#pragma unroll
            for (int k = 0; k < 12; ++k) m[i][k] = Mg[k];
        }
#pragma unroll
        for (int i = 0; i < NSRC; ++i) {
            const float* M = m[i];
            ray[i] = make_ray(M, xf, yf);
            T0[i] = M[3]; T1[i] = M[7]; T2[i] = M[11];
            // (kept in vector registers: as scalars they would be live across the whole planning prologue, and the scalar
            //  file is what spills into the plane loop -- one v_readlane per use)
            if constexpr (EARLY_INPUTS) asm volatile("" : "+v"(T0[i]), "+v"(T1[i]), "+v"(T2[i]));
        }
    };
    if constexpr (EARLY_INPUTS) projection_rows();
    f4 r[F16 ? 1 : Q];
    float rh[F16 ? Q : 1][8];   // fp16 storage: reference features of the group, 8 channels per chunk
    // (defer: the loaded values stay as they came -- finish_inputs() masks them after the planning.  Masking at once would wait
    //  for the loads where they are issued.)
    auto load_reference = [&](bool defer) {
        if (F16) {
#pragma unroll
            for (int q = 0; q < Q; ++q)
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    float t = ldf(reinterpret_cast<const T*>(p.feats[0]) + (size_t)(c0 + 8 * q + k) * plane + pix);
                    rh[F16 ? q : 0][k] = (defer || valid) ? t : 0.0f;
                }
        } else if (MODE != MODE_WARP) {
#pragma unroll
            for (int q = 0; q < Q; ++q)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float t = p.feats[0][(size_t)(c0 + 4 * q + k) * plane + pix];
                    r[F16 ? 0 : q][k] = (defer || valid) ? t : 0.0f;
                }
        }
    };
    float vw[NSRC];
    float rden = 0.0f;
    float aff_lo = 1.0f, aff_step = 0.0f;   // D3D_DEPTH_AFFINE: this lane's pixel
    auto finish_weights = [&]() {
        if (MODE == MODE_WEIGHTED) {
            float den = 1e-5f;
#pragma unroll
            for (int i = 0; i < NSRC; ++i) {
                vw[i] = (valid && i < p.n_src) ? vw[i] : 0.0f;
                den += vw[i];
            }
            rden = 1.0f / den;
        }
    };
    auto finish_inputs = [&]() {   // what a deferred lane_inputs() left undone: lanes outside the image carry zeros
        finish_weights();
        if (F16) {
#pragma unroll
            for (int q = 0; q < Q; ++q)
#pragma unroll
                for (int k = 0; k < 8; ++k) rh[F16 ? q : 0][k] = valid ? rh[F16 ? q : 0][k] : 0.0f;
        } else if (MODE != MODE_WARP) {
#pragma unroll
            for (int q = 0; q < Q; ++q)
#pragma unroll
                for (int k = 0; k < 4; ++k) r[F16 ? 0 : q][k] = valid ? r[F16 ? 0 : q][k] : 0.0f;
        }
    };
    auto lane_inputs = [&](bool defer) {
        if (MODE == MODE_WEIGHTED) {
#pragma unroll
            for (int i = 0; i < NSRC; ++i) vw[i] = p.weights[(size_t)min(i, p.n_src - 1) * plane + pix];
            if (!defer) finish_weights();
        }
        load_reference(defer);   // group 0
        if (p.depth_mode == D3D_DEPTH_AFFINE && valid) {
            aff_lo = p.depth[pix];
            aff_step = p.depth[plane + pix];
        }
    };
    if (EARLY_INPUTS && !loader) lane_inputs(true);

    // --- zero cell and per-plane depth range of this patch -------------------------------------
    for (int i = tid; i < 2 * STRIDE; i += THREADS) lds[L::ZERO + i] = 0.0f;
    if (p.depth_mode == D3D_DEPTH_PER_PLANE) {
        if (dtid >= 0 && dtid < nplanes) {
            lds[L::PMIN + dtid] = dplane;
            lds[L::PMAX + dtid] = dplane;
        }
    } else if (p.depth_mode == D3D_DEPTH_AFFINE) {
        // hypotheses lo + k * step per pixel (two maps): each lane reads its pixels' pair ONCE, the per-plane range of the patch
        // is arithmetic (the per-pixel form below re-reads the patch for every plane: a global-latency chain per plane)
        float blo[(TW * TH) / 64], bst[(TW * TH) / 64];
        bool bok[(TW * TH) / 64];
#pragma unroll
        for (int k = 0; k < (TW * TH) / 64; ++k) {
            const int q = lane + 64 * k;
            const int qx = x0 + (q & (PW - 1)), qy = y0 + (q >> pwsh);
            bok[k] = qx < w && qy < h;
            const size_t qi = bok[k] ? (size_t)qy * w + qx : 0;
            blo[k] = p.depth[qi];
            bst[k] = p.depth[plane + qi];
        }
        for (int i = wave; i < nplanes; i += NWAVES) {
            float lo = INFINITY, hi = -INFINITY;
#pragma unroll
            for (int k = 0; k < (TW * TH) / 64; ++k) {
                const float dv = __fadd_rn(blo[k], __fmul_rn((float)(ds + i), bst[k]));
                if (bok[k]) { lo = fminf(lo, dv); hi = fmaxf(hi, dv); }
            }
            lo = wave_min(lo);
            hi = wave_max(hi);
            if (lane == 0) {
                lds[L::PMIN + i] = lo;
                lds[L::PMAX + i] = hi;
            }
        }
    } else {
        for (int i = wave; i < nplanes; i += NWAVES) {
            float lo = INFINITY, hi = -INFINITY;
#pragma unroll
            for (int k = 0; k < (TW * TH) / 64; ++k) {
                int q = lane + 64 * k;
                int qx = x0 + (q & (PW - 1)), qy = y0 + (q >> pwsh);
                if (qx < w && qy < h) {
                    float dv = p.depth[(size_t)(ds + i) * plane + (size_t)qy * w + qx];
                    lo = fminf(lo, dv);
                    hi = fmaxf(hi, dv);
                }
            }
            lo = wave_min(lo);
            hi = wave_max(hi);
            if (lane == 0) {
                lds[L::PMIN + i] = lo;
                lds[L::PMAX + i] = hi;
            }
        }
    }
    __syncthreads();
    const long long t_range = D3D_CLOCK();

    // --- plan every step of the segment ---------------------------------------------------------
    // One wave per source view (wave i plans view i; the other waves only follow the barriers):
    // P1:  the view's windows for the candidate step sizes m in {4, 2, 1}, ALL candidates in one pass -- one lane per (candidate,
    //      step): 8 + 16 + 32 lanes for a 128-plane segment; results go to a scratch table in the (still unused) ring area.
    // P2a: every wave picks the largest candidate whose rings fit (the same few words, read by all); the view's wave writes the
    //      view's plan entries and ring geometry and cuts the view's window deltas into rectangles, whose counts go to scratch.
    // P2b: the view's wave sums the counts of all views (the scan over the steps is repeated per view: 6 shuffles, on another
    //      SIMD each), and writes the view's rectangle descriptors; wave 0 also writes the step tables and the header.
    // The tables hold the same words as when one wave built them view after view.
    static_assert(NWAVES >= NSRC, "one planning wave per source view");
    typedef int i4v __attribute__((ext_vector_type(4)));
    typedef int i2v __attribute__((ext_vector_type(2)));
    constexpr int CT = L::DATA;                          // [cand][view][step][4] windows
    constexpr int CHD = CT + NCAND * NSRC * 64 * 4;      // [cand][view][4]: RW, RH, bad, nsteps
    constexpr int CNT = CHD + NCAND * NSRC * 4;          // [view][step][2]: non-empty delta rectangles, positions to stage
    constexpr int FLG = CNT + NSRC * 64 * 2;             // [cand]: 1 = the candidate's staging work fits the descriptors
    // candidate c steps by NSUB*4, NSUB*2, NSUB, NSUB/2 planes (the last leaves half the sub-waves idle,
    // which is still far better than gathering from global memory)
    auto cand_planes = [](int c) { return c < 3 ? NSUB * (4 >> c) : max(NSUB / 2, 1); };
    auto cand_steps = [&](int c) { const int SPc = cand_planes(c); return (nplanes + SPc - 1) / SPc; };
    // windows of view vsel for the candidates [c_lo, c_hi), whose steps share the wave's lanes: candidate c_lo's first, then the
    // next one's (the caller has checked that they fit 64 lanes; an infeasible candidate takes none)
    auto candidate_windows = [&](int c_lo, int c_hi, int vsel) {
        {
            int myc = -1, st = 0;
            for (int c = c_lo, off = 0; c < c_hi; ++c) {
                const int n = cand_steps(c) <= MAXSTEPS ? cand_steps(c) : 0;
                if (lane >= off && lane < off + n) { myc = c; st = lane - off; }
                off += n;
            }
            const bool act = myc >= 0;
            const int SPc = cand_planes(act ? myc : c_lo);
            const int p0 = min(st * SPc, nplanes - 1), p1 = min(st * SPc + SPc, nplanes);
            // depth range of the step's planes: independent reads (an index past the step repeats its last plane: min and max
            // are exact and idempotent, so the range has the same bits as a loop over [p0, p1) has)
            float lo = INFINITY, hi = -INFINITY;
#pragma unroll
            for (int j = 0; j < NSUB * 4; ++j) {
                const int i = min(p0 + j, p1 - 1);
                lo = fminf(lo, lds[L::PMIN + i]);
                hi = fmaxf(hi, lds[L::PMAX + i]);
            }
            const float* M = mw;   // (vsel is this wave's view: rows of p.proj34 + 12 * min(vsel, p.n_src - 1), requested at the top)
            float umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY;
            bool ok = true;
#pragma unroll
            for (int ck = 0; ck < 8; ++ck) {
                Ray cr = make_ray(M, (ck & 1) ? (float)x1c : (float)x0, (ck & 2) ? (float)y1c : (float)y0);
                const float dv = (ck & 4) ? hi : lo;
                float qx = __fadd_rn(__fmul_rn(cr.rx, dv), M[3]);
                float qy = __fadd_rn(__fmul_rn(cr.ry, dv), M[7]);
                float qz = __fadd_rn(__fmul_rn(cr.rz, dv), M[11]);
                ok = ok && (qz > 1e-20f) && (qz < 1e30f);
                float iz = 1.0f / qz;
                float u = qx * iz, v = qy * iz;
                ok = ok && (fabsf(u) < 1e30f) && (fabsf(v) < 1e30f);
                // the same clamp as the samples' (geo_ring): windows lie in [-1, w + 1] x [-1, h + 1]
                u = fminf(fmaxf(u, -1.0f), (float)w);
                v = fminf(fmaxf(v, -1.0f), (float)h);
                umin = fminf(umin, u); umax = fmaxf(umax, u);
                vmin = fminf(vmin, v); vmax = fmaxf(vmax, v);
            }
            // interior samples differ from the corner hull by fp32 rounding only (<< 1/16 px)
            int wx0 = max((int)floorf(umin - 0.0625f), -1);
            int wy0 = max((int)floorf(vmin - 0.0625f), -1);
            int wx1 = min((int)floorf(umax + 0.0625f) + 1, w + 1);
            int wy1 = min((int)floorf(vmax + 0.0625f) + 1, h + 1);
            int ww = max(wx1 - wx0 + 1, 0), wh = max(wy1 - wy0 + 1, 0);   // >= 2 x 2: every sample has its four taps in the window
            // unused view of the template (n_src < NSRC): its samples sit at (-1, -1) (geo_ring with a zero ray), weight 1 on
            // the tap at (-1, -1) -- a zero -- and weight 0 on the other three (pixel (0, 0) among them: zero_first_cells_kernel)
            if (vsel >= p.n_src) { wx0 = -1; wy0 = -1; ww = 2; wh = 2; ok = true; }
            if (!act) { ww = 0; wh = 0; ok = true; }
            // ring size: the union of consecutive windows must fit (asynchronous delta staging)
            int ux = ww, uy = wh;
            {
                const int qx0 = __shfl_up(wx0, 1), qy0 = __shfl_up(wy0, 1);
                const int qw = __shfl_up(ww, 1), qh = __shfl_up(wh, 1);
                if (st > 0 && act && qw > 0 && ww > 0) {   // (st > 0: the lane below holds the candidate's previous step)
                    ux = max(wx0 + ww, qx0 + qw) - min(wx0, qx0);
                    uy = max(wy0 + wh, qy0 + qh) - min(wy0, qy0);
                }
            }
            if (act) *reinterpret_cast<i4v*>(ldsi + CT + ((myc * NSRC + vsel) * 64 + st) * 4) = (i4v){wx0, wy0, ww, wh};
            // ring size and "bad" flag of each candidate: maxima over its lanes, taken by the LDS (a wave's LDS instructions
            // execute in order: lane 0's initial words are there before the first maximum arrives)
            if (lane == 0)
                for (int c = c_lo; c < c_hi; ++c)
                    *reinterpret_cast<i4v*>(ldsi + CHD + (c * NSRC + vsel) * 4) = (i4v){1, 1, cand_steps(c) > MAXSTEPS ? 1 : 0, cand_steps(c)};
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            if (act) {
                int* hd = ldsi + CHD + (myc * NSRC + vsel) * 4;
                atomicMax(hd + 0, ux);
                atomicMax(hd + 1, uy);
                if (!ok) atomicOr(hd + 2, 1);  // p.z <= 0 somewhere: cannot bound the frustum
            }
        }
    };
    long long t_p1 = 0;
    // One planning round over the candidates [cbeg, cend): every wave runs it (the same barriers), returns 1 when the rings are planned.
    auto plan_round = [&](int cbeg, int cend) -> int {
        if (wave < NSRC) {
            int lanes = 0;
            for (int c = cbeg; c < cend; ++c) lanes += cand_steps(c) <= MAXSTEPS ? cand_steps(c) : 0;
            if (lanes <= 64) {
                candidate_windows(cbeg, cend, wave);
            } else {   // (segments longer than any launched: one candidate at a time)
                for (int c = cbeg; c < cend; ++c) candidate_windows(c, c + 1, wave);
            }
        }
        __syncthreads();
        if (cbeg == 0) t_p1 = D3D_CLOCK();
        int mode = 0, sp_sel = NSUB, nsteps_sel = (nplanes + NSUB - 1) / NSUB;
        for (int cand = cbeg; cand < cend && !mode; ++cand) {   // first candidate whose rings fit and whose deltas can be described
            const int nsteps = rfl(ldsi[CHD + (cand * NSRC) * 4 + 3]);
            const bool act = lane < nsteps;
            int RW[NSRC], RH[NSRC];
            int bad = 0, total = 0, totalq = 0;
            int RWq[NSRC], RHq[NSRC];   // rounded up for the bank layout (any size >= the union span is valid)
#pragma unroll
            for (int i = 0; i < NSRC; ++i) {
                const i4v hd = *reinterpret_cast<const i4v*>(ldsi + CHD + (cand * NSRC + i) * 4);
                RW[i] = rfl(hd[0]); RH[i] = rfl(hd[1]); bad |= rfl(hd[2]);
                RWq[i] = (RW[i] + RING_RW_QUANT - 1) / RING_RW_QUANT * RING_RW_QUANT;
                RHq[i] = (RH[i] + RING_RH_QUANT - 1) / RING_RH_QUANT * RING_RH_QUANT;
                total += ring_row_floats<STRIDE>(RW[i]) * (RH[i] + 1);
                totalq += ring_row_floats<STRIDE>(RWq[i]) * (RHq[i] + 1);
            }
            if (totalq <= a.cap_floats) {   // the conflict-free ring sizes fit: use them
                total = totalq;
#pragma unroll
                for (int i = 0; i < NSRC; ++i) { RW[i] = RWq[i]; RH[i] = RHq[i]; }
            }
            if (bad || total > a.cap_floats) continue;
            sp_sel = cand_planes(cand);
            nsteps_sel = nsteps;
            // this wave's view: its ring (the rings follow each other from L::DATA on)
            int RWv = 1, RHv = 1, basev = L::DATA;
            bool dims_ok = true;
            {
                int base = L::DATA;
#pragma unroll
                for (int i = 0; i < NSRC; ++i) {
                    if (i == wave) { RWv = RW[i]; RHv = RH[i]; basev = base; }
                    dims_ok = dims_ok && RW[i] < 256 && RH[i] < 256;
                    base += ring_row_floats<STRIDE>(RW[i]) * (RH[i] + 1);
                }
            }
            int wx0 = 0, wy0 = 0, oxv = 0, oyv = 0;
            int rx[4], ry[4], rwid[4], nel[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) { rx[r] = 0; ry[r] = 0; rwid[r] = 0; nel[r] = 0; }
            if (wave < NSRC) {
                const int vi = wave;
                const i4v e = *reinterpret_cast<const i4v*>(ldsi + CT + ((cand * NSRC + vi) * 64 + lane) * 4);
                // (lanes past the last step hold no window: they stage nothing and write no entry)
                wx0 = act ? e[0] : 0; wy0 = act ? e[1] : 0;
                const int ww = act ? e[2] : 0, wh = act ? e[3] : 0;
                // ring coordinates are taken relative to the first step's window origin
                const int cx0 = __shfl(wx0, 0), cy0 = __shfl(wy0, 0);
                oxv = posmod(wx0 - cx0, RWv);
                oyv = posmod(wy0 - cy0, RHv);
                if (act) {
                    int* pe = ldsi + L::PLAN + (lane * NSRC + vi) * 8;
                    *reinterpret_cast<i4v*>(pe) = (i4v){wx0, wy0, ww, wh};
                    // oxv - wx0: ring column of source column 0 (geo_ring's kx, ky)
                    *reinterpret_cast<i4v*>(pe + 4) = (i4v){oxv, oyv, oxv - wx0, oyv - wy0};
                }
                if (lane == 0) {
                    *reinterpret_cast<i4v*>(ldsi + L::HDR + 4 + 4 * vi) = (i4v){RWv, RHv, basev, RWv | (RHv << 8) | ((basev >> 2) << 16)};
                    if constexpr (VIEW_MAJOR) {   // the plane loop reads its per-view constants back from here (see `geometry`)
                        const float* __restrict__ M = p.proj34 + 12 * min(vi, p.n_src - 1);
                        const bool dummy = vi >= p.n_src;   // unused view of the template: every sample at (-1, -1)
                        lds[L::VT + 8 * vi + 0] = dummy ? -1.0f : M[3];
                        lds[L::VT + 8 * vi + 1] = dummy ? -1.0f : M[7];
                        lds[L::VT + 8 * vi + 2] = dummy ? 1.0f : M[11];
                        lds[L::VT + 8 * vi + 3] = 0.0f;
                        ldsi[L::VT + 8 * vi + 4] = RWv;
                        ldsi[L::VT + 8 * vi + 5] = RHv;
                        ldsi[L::VT + 8 * vi + 6] = ring_row_floats<STRIDE>(RWv) * 4;
                        ldsi[L::VT + 8 * vi + 7] = lds_base_bytes(lds) + 4 * basev;
                    }
                }
                // ---- staging items of every step: window(k) minus window(k-1) as <= 4 rectangles per
                // view, cut into items of 64 positions (all CH channels of the group).
                const int xa = wx0, xb = wx0 + ww - 1, ya = wy0, yb = wy0 + wh - 1;
                const int pxa = __shfl_up(wx0, 1), pya = __shfl_up(wy0, 1);
                const int pxb = pxa + __shfl_up(ww, 1) - 1, pyb = pya + __shfl_up(wh, 1) - 1;
                int ix0 = 1, ix1 = 0, iy0 = 1, iy1 = 0;  // intersection with the previous window
                if (lane > 0) { ix0 = max(xa, pxa); ix1 = min(xb, pxb); iy0 = max(ya, pya); iy1 = min(yb, pyb); }
                const bool ov = (ix0 <= ix1) && (iy0 <= iy1);
                // left | right | top | bottom; without overlap "left" is the whole window
                int rh_[4];
                rx[0] = xa;      ry[0] = ya;      rwid[0] = (ov ? ix0 - 1 : xb) - xa + 1; rh_[0] = wh;
                rx[1] = ix1 + 1; ry[1] = ya;      rwid[1] = ov ? xb - ix1 : 0;             rh_[1] = wh;
                rx[2] = ix0;     ry[2] = ya;      rwid[2] = ov ? ix1 - ix0 + 1 : 0;        rh_[2] = ov ? iy0 - ya : 0;
                rx[3] = ix0;     ry[3] = iy1 + 1; rwid[3] = ov ? ix1 - ix0 + 1 : 0;        rh_[3] = ov ? yb - iy1 : 0;
                int nrect_v = 0, npos_v = 0;   // non-empty rectangles | positions this view stages in the step
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    nel[r] = act ? max(rwid[r], 0) * max(rh_[r], 0) : 0;
                    nrect_v += nel[r] > 0 ? 1 : 0;
                    npos_v += nel[r];
                }
                *reinterpret_cast<i2v*>(ldsi + CNT + (vi * 64 + lane) * 2) = (i2v){nrect_v, npos_v};
            }
            __syncthreads();
            if (wave < NSRC) {
                const int vi = wave;
                int nrect = 0, npos = 0;     // of the step, all views
                int idx = 0, pstart = 0;     // of the views before this one
#pragma unroll
                for (int i = 0; i < NSRC; ++i) {
                    const i2v c = *reinterpret_cast<const i2v*>(ldsi + CNT + (i * 64 + lane) * 2);
                    nrect += c[0]; npos += c[1];
                    if (i < vi) { idx += c[0]; pstart += c[1]; }
                }
                // scan over the steps, bit by bit of the counts (<= 4 * NSRC < 32): a ballot and a count of the lanes below per bit,
                // no trip through the LDS crossbar
                int incl = nrect, total_rects = 0;
#pragma unroll
                for (int bit = 0; bit < 5; ++bit) {
                    const unsigned long long m = __ballot((nrect >> bit) & 1);
                    incl += (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u)) << bit;
                    total_rects += __popcll(m) << bit;
                }
                // (field widths of the descriptors: a step stages < 65536 positions, windows are < 4096 wide)
                // if they do not hold: cannot describe the staging work -- the next candidate, or gather from global memory instead
                const bool fits = !(total_rects > MAXRECTS || !dims_ok || __any(npos > 0xffff) || w > 0xfff0 || h > 0xfff0);
                if (fits) {
                    idx += incl - nrect;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (nel[r] > 0) {
                            *reinterpret_cast<i4v*>(ldsi + L::RECTS + 4 * idx) =
                                (i4v){(rx[r] + 1) | ((ry[r] + 1) << 16),   // windows start at >= -1
                                      rwid[r] | (vi << 12) | (pstart << 16),
                                      nel[r],
                                      // ring coordinates of the rect origin (unwrapped: < 2*RW, 2*RH)
                                      (rx[r] - wx0 + oxv) | ((ry[r] - wy0 + oyv) << 16)};
                            pstart += nel[r];
                            ++idx;
                        }
                    if (vi == 0) {
                        if (act) {
                            ldsi[L::SST + lane] = incl - nrect;
                            ldsi[L::STOT + lane] = npos;
                        }
                        if (lane == nsteps - 1) ldsi[L::SST + nsteps] = incl;
                        if (lane == 0) {
                            ldsi[L::HDR + 0] = 1;
                            ldsi[L::HDR + 1] = sp_sel;
                            ldsi[L::HDR + 2] = nsteps_sel;
                        }
                    }
                }
                if (vi == 0 && lane == 0) ldsi[FLG + cand] = fits ? 1 : 0;
            }
            __syncthreads();
            mode = rfl(ldsi[FLG + cand]);
        }
        if (!mode) {   // (workgroup-uniform) no rings: the header says so, with the step of the last candidate that fitted, if any
            if (tid == 0) {
                ldsi[L::HDR + 0] = 0;
                ldsi[L::HDR + 1] = sp_sel;
                ldsi[L::HDR + 2] = nsteps_sel;
            }
            __syncthreads();
        }
        return mode;
    };
    // the three regular candidates first; the half-step candidate only when none of them fits (rare: very wide plane spacing)
    constexpr int NCAND1 = NCAND - 1;
    if (plan_round(0, NCAND1) == 0) plan_round(NCAND1, NCAND);
    if (D3D_STAMPS && a.tstats && tid == 0) {  // prologue phases: depth range | windows of every candidate | plan + rectangle tables
        const long long t_p2 = clock64();
        atomicAdd(a.tstats + 16, (unsigned long long)(t_range - t_start));
        atomicAdd(a.tstats + 17, (unsigned long long)(t_p1 - t_range));
        atomicAdd(a.tstats + 18, (unsigned long long)(t_p2 - t_p1));
    }
    const int ring = rfl(ldsi[L::HDR + 0]);
    const int SP = rfl(ldsi[L::HDR + 1]);  // planes per step
    const int nsteps = rfl(ldsi[L::HDR + 2]);
    if (D3D_STAMPS && a.stats && tid == 0) {
        atomicAdd(a.stats + (ring ? 0 : 1), 1u);
        atomicAdd(a.stats + 2, (unsigned)SP);
        atomicAdd(a.stats + 3, (unsigned)nsteps);
        if (ring) {
            unsigned tot = 0;
            for (int i = 0; i < NSRC; ++i) tot += (ldsi[L::HDR + 4 + 4 * i] + 1) * (ldsi[L::HDR + 5 + 4 * i] + 1);
            atomicAdd(a.stats + 4, tot);
        }
    }
    // ---------------------------------------------------------------------------------------
    // Delta staging: step k owns the rectangle descriptors [sst[k], sst[k+1]), whose positions are cut into items of 64;
    // wave sw of the snw waves that share the step takes the items sw, sw + snw, ..., PFD of them per round: the loads of
    // a round are all requested before the first of them is written to the rings.  Step k + 1 is staged while step k is swept.
    // ---------------------------------------------------------------------------------------
    struct Item {
        const float* g;  // global address of the group's first channel (always dereferenceable)
        int meta;        // LDS float index of the ring slot | ok << 20 | dup column << 21 | dup row << 22, or -1
        int geo;         // RW | RH << 8 of the view's ring
    };
    long long fdelta[NSRC];  // byte distance from the first source map to source map i (wave-uniform)
#pragma unroll
    for (int i = 0; i < NSRC; ++i) {
        const long long d0 = reinterpret_cast<long long>(p.feats[1]);
        const long long di = reinterpret_cast<long long>(p.feats[i + 1]);
        fdelta[i] = (i < p.n_src) ? di - d0 : 0;
    }
    // Element `el` (0..T-1) of step k's flattened delta -> source address and ring slot of this lane.
    // Each lane finds its own rectangle (<= 16 per step), so items are densely packed.
    auto item = [&](int el, int Tn, int rb, const int (&pst16)[MAXRS]) -> Item {
        Item I;
        const bool live = el < Tn;
        // rect holding element el: count the rect starts <= el (starts beyond the step's rects are INT_MAX)
        int ridx = rb - 1;
#pragma unroll
        for (int rr = 0; rr < MAXRS; ++rr) ridx += (pst16[rr] <= el) ? 1 : 0;
        ridx = max(ridx, rb);
        const int* e = ldsi + L::RECTS + 4 * ridx;
        const int e0 = e[0], e1 = e[1], e6 = e[3];
        const int rx = (e0 & 0xffff) - 1, ry = (e0 >> 16) - 1;
        const int rwid = e1 & 0xfff, vi = (e1 >> 12) & 0xf, pst = (unsigned)e1 >> 16;
        const int e7 = ldsi[L::HDR + 4 + 4 * vi + 3];   // ring geometry of the rect's view
        const int RWv = e7 & 0xff, RHv = (e7 >> 8) & 0xff, bs = (e7 >> 16) << 2;
        const int pos = el - pst;
        const int cy = (int)(((float)pos + 0.5f) * __builtin_amdgcn_rcpf((float)max(rwid, 1)));
        const int cx = pos - cy * rwid;
        const int sx = rx + cx, sy = ry + cy;
        const bool ok = live && ((unsigned)sx < (unsigned)w) && ((unsigned)sy < (unsigned)h);
        // per-lane source view: feats[1] + (uniform) byte distance to view vi's map.  Kept as integer
        // arithmetic on purpose: a select chain over the pointers is turned back into an indexed load
        // of the argument block, whose s_waitcnt vmcnt(0) would serialise the staging loads.
        long long dsel = 0;
#pragma unroll
        for (int i = 1; i < NSRC; ++i) dsel = (vi == i) ? fdelta[i] : dsel;
        if (a.cl)  // one position's CH channels are contiguous: 16-byte loads
            I.g = a.cl + ((size_t)(vi * a.ngroups + grp) * plane + (size_t)(ok ? sy * w + sx : 0)) * CW;
        else
            I.g = reinterpret_cast<const float*>(reinterpret_cast<const char*>(p.feats[1]) + dsel) + (size_t)c0 * plane +
                  (ok ? sy * w + sx : 0);
        unsigned c = (unsigned)((e6 & 0xffff) + cx), r = (unsigned)((e6 >> 16) + cy);
        c = min(c, c - (unsigned)RWv);
        r = min(r, r - (unsigned)RHv);
        const int dst = bs + (int)r * ring_row_floats<STRIDE>(RWv) + (int)c * STRIDE;
        I.meta = live ? (dst | (ok ? 1 << 20 : 0) | (c == 0 ? 1 << 21 : 0) | (r == 0 ? 1 << 22 : 0)) : -1;
        I.geo = e7 & 0xffff;
        return I;
    };
    auto put = [&](int meta, int geo, int q, f4 v) {
        if (meta >= 0) {
            const int dst = (meta & 0xfffff) + 4 * q;
            const int RWv = geo & 0xff, RHv = geo >> 8;
            const int dupc = (meta >> 21) & 1 ? RWv * STRIDE : 0;
            const int dupr = (meta >> 22) & 1 ? RHv * ring_row_floats<STRIDE>(RWv) : 0;
            f4 x = (meta >> 20) & 1 ? v : (f4){0, 0, 0, 0};
            *reinterpret_cast<f4*>(lds + dst) = x;
            if (dupc) *reinterpret_cast<f4*>(lds + dst + dupc) = x;
            if (dupr) *reinterpret_cast<f4*>(lds + dst + dupr) = x;
            if (dupc && dupr) *reinterpret_cast<f4*>(lds + dst + dupc + dupr) = x;
        }
    };
    // A staging item that lies inside ONE rectangle (all but the items of the thin L-shaped deltas) is decoded once per wave:
    // the descriptor and the view's ring geometry are wave-uniform, so they are unpacked in scalar registers and a lane is left
    // with pos -> (cx, cy), its source offset (32 bits against a wave-uniform base) and its ring slot.  Same arithmetic per
    // position as item(), so the rings hold the same bytes whichever path staged them.
    // Whether all of the item lies inside the image and none of it in ring column 0 or ring row 0 is decided in scalar code too:
    // kind 0: it does -- the loaded values are written as they are, once (meta = ring slot, or -1 past the end of the delta);
    // kind 1: meta carries the ok | duplicate-column | duplicate-row flags and put() honours them (every generic item too).
    // (Sparing the selects and the duplicate writes SEPARATELY -- most one-rectangle items are inside the image but meet ring
    //  column 0 or row 0 -- cut 1.5 % more vector instructions and lost the time the decode had won: profiles/loader_decode_ab.txt.)
    // Not in the shallow form (32 x 8 patches, sweeps of at most 16 planes): its staging is one first window per pass, and the
    // 8-plane stage of the cascade ran 2 % slower with this path than without (profiles/loader_decode_ab.txt, section 6).
    constexpr bool ONE_RECT = NPIXW <= 2;
    struct Rects {   // lane rr < MAXRS: descriptor words of the step's rr-th rectangle and the ring geometry word of its view
        int psv, d0, d1, d3, d7;
    };
    // 32-bit source offsets reach every channel of every position (planar: 4 * CH planes; channel-last: CW words per position)
    const bool small32 = plane <= (size_t)0xffffffffu / (size_t)(CH * 4 > 64 ? CH * 4 : 64);
    f4 pf[PFD][Q];
    int pmeta[PFD], pgeo[PFD];
    int pkind[PFD];   // wave-uniform
    auto write_round = [&]() {
#pragma unroll
        for (int j = 0; j < PFD; ++j) {
            if (pkind[j] == 0) {
                if (pmeta[j] >= 0) {
#pragma unroll
                    for (int q = 0; q < Q; ++q) *reinterpret_cast<f4*>(lds + pmeta[j] + 4 * q) = pf[j][q];
                }
            } else {
#pragma unroll
                for (int q = 0; q < Q; ++q) put(pmeta[j], pgeo[j], q, pf[j][q]);
            }
        }
    };
    // Loader waves: bring window(k) minus window(k-1) into the rings.
    const bool ltiming = D3D_STAMPS && a.tstats != nullptr && lw == 0;
    long long lt_issue = 0, lt_write = 0, lt_bar = 0;
    // (sw, snw): this wave's index among the snw waves sharing the step's items -- the loaders for the deltas;
    // ALL waves for the initial window, which nothing can overlap (one workgroup per CU): the compute waves
    // would only wait for it.
    auto stage = [&](int k, int sw, int snw) {
        const int rb = rfl(ldsi[L::SST + k]), re = rfl(ldsi[L::SST + k + 1]);
        const int Tn = rfl(ldsi[L::STOT + k]);
        const int nitems = (Tn + 63) >> 6;
        // the step's (<= 4 per view) rects, one per lane: first positions (wave-uniform copies for item()), and the
        // descriptors the one-rectangle items read back with v_readlane
        Rects R;
        {
            const bool have = lane < re - rb;
            const int* e = ldsi + L::RECTS + 4 * (rb + min(lane, MAXRS - 1));
            R.d1 = e[1];
            R.psv = have ? (int)((unsigned)R.d1 >> 16) : 0x7fffffff;
            if constexpr (ONE_RECT) {
                R.d0 = e[0]; R.d3 = e[3];
                R.d7 = ldsi[L::HDR + 4 + 4 * (have ? (R.d1 >> 12) & 0xf : 0) + 3];
            } else {
                R.d0 = R.d3 = R.d7 = 0;
            }
        }
        const int psv = R.psv;
        int pst16[MAXRS];
#pragma unroll
        for (int rr = 0; rr < MAXRS; ++rr) pst16[rr] = __builtin_amdgcn_readlane(psv, rr);
        unsigned n_items = 0, n_one = 0, n_plain = 0, n_in = 0, n_nodup = 0, n_idle = 0;   // (D3D_TILED_STATS)
        for (int it0 = sw; it0 < nitems; it0 += snw * PFD) {
            long long tq1 = 0, tq2 = 0;
            if (ltiming) tq1 = clock64();
#pragma unroll
            for (int j = 0; j < PFD; ++j) {
                const int it = it0 + snw * j;
                int meta = -1, geo = 0, kind = 0;   // (no item left for this slot of the round: nothing to write)
                f4 v[Q];
                if (it < nitems) {
                    const int el0 = it * 64;
                    const int nlive = min(Tn - el0, 64);   // >= 1
                    // no rectangle starts inside (el0, el0 + nlive): the live elements share the rectangle of el0
                    const bool one = ONE_RECT && __ballot(psv > el0 && psv < el0 + nlive) == 0ull;
                    if (D3D_STAMPS) { ++n_items; n_one += one ? 1 : 0; }
                    if (one && small32) {
                        const int rsel = max(__popcll(__ballot(psv <= el0)) - 1, 0);
                        const int e0 = __builtin_amdgcn_readlane(R.d0, rsel), e1 = __builtin_amdgcn_readlane(R.d1, rsel);
                        const int e6 = __builtin_amdgcn_readlane(R.d3, rsel), e7 = __builtin_amdgcn_readlane(R.d7, rsel);
                        const int rx = (e0 & 0xffff) - 1, ry = (e0 >> 16) - 1;
                        const int rwid = e1 & 0xfff, vi = (e1 >> 12) & 0xf, pst = (int)((unsigned)e1 >> 16);
                        const int RWv = e7 & 0xff, RHv = (e7 >> 8) & 0xff, bs = (e7 >> 16) << 2;
                        const int oc = e6 & 0xffff, orow = e6 >> 16;   // ring column / row of the rect origin (unwrapped)
                        const bool live = lane < nlive;
                        const int pos = (el0 - pst) + lane;
                        const int cy = (int)(((float)pos + 0.5f) * __builtin_amdgcn_rcpf((float)max(rwid, 1)));
                        const int cx = pos - (int)__mul24(cy, rwid);
                        // rectangle rows the live elements cover (lane 0 is always live)
                        const int cya = rfl(cy), cyb = __builtin_amdgcn_readlane(cy, nlive - 1);
                        const bool inside = rx >= 0 && rx + rwid <= w && ry + cya >= 0 && ry + cyb < h;
                        // ring column 0 / row 0 are met at the unwrapped coordinates 0 and RW / RH
                        const bool dups = oc == 0 || (oc <= RWv && RWv < oc + rwid) || orow + cya == 0 ||
                                          (orow + cya <= RHv && RHv <= orow + cyb);
                        const int sx = rx + cx, sy = ry + cy;
                        unsigned c = (unsigned)(oc + cx), r = (unsigned)(orow + cy);
                        c = min(c, c - (unsigned)RWv);
                        r = min(r, r - (unsigned)RHv);
                        const int dst = bs + (int)__umul24(r, (unsigned)ring_row_floats<STRIDE>(RWv)) + (int)__umul24(c, (unsigned)STRIDE);
                        bool ok = live;
                        if (inside && !dups) {
                            meta = live ? dst : -1;
                        } else {
                            if (!inside) ok = live && ((unsigned)sx < (unsigned)w) && ((unsigned)sy < (unsigned)h);
                            meta = live ? (dst | (ok ? 1 << 20 : 0) | (c == 0 ? 1 << 21 : 0) | (r == 0 ? 1 << 22 : 0)) : -1;
                            geo = e7 & 0xffff;
                            kind = 1;
                        }
                        if (D3D_STAMPS) { n_plain += kind == 0 ? 1 : 0; n_in += inside ? 1 : 0; n_nodup += dups ? 0 : 1; }
                        const unsigned soff = ok ? __umul24((unsigned)sy, (unsigned)w) + (unsigned)sx : 0u;
                        if (a.cl) {
                            const char* gb = reinterpret_cast<const char*>(a.cl + (size_t)(vi * a.ngroups + grp) * plane * CW);
                            const f4* __restrict__ g = reinterpret_cast<const f4*>(gb + (size_t)(soff * (unsigned)(CW * 4)));
#pragma unroll
                            for (int q = 0; q < Q; ++q) v[q] = g[q];
                        } else if (!F16) {
                            long long dsel = 0;
#pragma unroll
                            for (int i = 1; i < NSRC; ++i) dsel = (vi == i) ? fdelta[i] : dsel;
                            const char* gb = reinterpret_cast<const char*>(p.feats[1]) + dsel + (size_t)c0 * plane * 4;
#pragma unroll
                            for (int q = 0; q < Q; ++q)
#pragma unroll
                                for (int kk = 0; kk < 4; ++kk)
                                    v[q][kk] = *reinterpret_cast<const float*>(gb + (size_t)(4 * q + kk) * plane * 4 + (size_t)(soff * 4u));
                        }
                    } else {
                        Item I = item(el0 + lane, Tn, rb, pst16);
                        if (a.cl) {
#pragma unroll
                            for (int q = 0; q < Q; ++q) v[q] = reinterpret_cast<const f4*>(I.g)[q];
                        } else if (!F16) {   // planar fp32 maps (no workspace given); fp16 rings are only launched with the channel-last copy
#pragma unroll
                            for (int q = 0; q < Q; ++q) {
                                const float* __restrict__ g = I.g + (size_t)(4 * q) * plane;
                                v[q][0] = g[0];
                                v[q][1] = g[plane];
                                v[q][2] = g[2 * plane];
                                v[q][3] = g[3 * plane];
                            }
                        }
                        meta = I.meta;
                        geo = I.geo;
                        kind = 1;
                    }
                } else if (D3D_STAMPS) {
                    ++n_idle;
                }
                pmeta[j] = meta;
                pgeo[j] = geo;
                pkind[j] = kind;
#pragma unroll
                for (int q = 0; q < Q; ++q) pf[j][q] = v[q];
            }
            if (ltiming) { tq2 = clock64(); lt_issue += tq2 - tq1; }
            write_round();
            if (ltiming) lt_write += clock64() - tq2;
        }
        if (D3D_STAMPS && a.stats && lane == 0) {
            atomicAdd(a.stats + 5, n_items);
            atomicAdd(a.stats + 6, n_one);
            atomicAdd(a.stats + 7, n_plain);
            atomicAdd(a.stats + 8, n_in);
            atomicAdd(a.stats + 9, n_nodup);
            atomicAdd(a.stats + 10, n_idle);
        }
    };

    // Barrier k separates {compute step k-1, stage delta k} from {compute step k, stage delta k+1}.
    // Both roles execute exactly nsteps barriers in ring mode and none in gather mode.
    // (In gather mode -- rings do not fit, or p.z <= 0 at a corner -- there is nothing to stage: the loader waves sweep
    //  planes too, see GATHER_ALL below.)
    if (loader && ring) {
        // (Raising the loaders' issue priority with s_setprio was measured: their decode time halves,
        // but the compute waves lose the same slots and the kernel gets 5 % slower -- left at default.)
        for (int gi = 0; gi < a.ngroups; ++gi) {
            grp = gi;
            c0 = gi * CH;
            // First window of a pass: every wave of the workgroup stages it, the compute waves too.  Neutral on deep sweeps (239k
            // cycles per workgroup either way), -7 % on the cascade's 8-plane stage where that window is the only staging there is.
            if (ring) {   // (always true here.  Without it the compiler inverts one loop branch: kept so that deleting the experiment paths
                          //  left every kernel's machine code byte-identical)
                stage(0, wave, NWAVES);
                for (int k = 0; k < nsteps; ++k) {
                    long long tb = 0;
                    if (ltiming) tb = clock64();
                    __syncthreads();
                    if (ltiming) lt_bar += clock64() - tb;
                    if (k + 1 < nsteps) stage(k + 1, lw, NLOADW);
                }
            }
            __syncthreads();  // end of the pass: the rings may be overwritten with the next group's first window
        }
        if (ltiming && lane == 0) {
            atomicAdd(a.tstats + 2, (unsigned long long)lt_bar);
            atomicAdd(a.tstats + 6, (unsigned long long)lt_issue);
            atomicAdd(a.tstats + 7, (unsigned long long)lt_write);
        }
        return;
    }

    // --- per-lane constants: rays, reference features, weights -------------------------------
    if constexpr (!EARLY_INPUTS) {
        projection_rows();
        lane_inputs(false);
    } else {
        if (loader) lane_inputs(false);   // (gather mode: the loader waves sweep planes, and skipped their inputs above)
        else finish_inputs();
    }
    RingView RV[NSRC];
    const int lds0 = lds_base_bytes(lds);
    const float umax = (float)w, vmax = (float)h;   // geo_ring's clamp bounds
#pragma unroll
    for (int i = 0; i < NSRC; ++i) {
        if (ring && i >= p.n_src) {   // unused view of the template: every sample at (-1, -1), see the planner
            ray[i].rx = 0.0f; ray[i].ry = 0.0f; ray[i].rz = 0.0f;
            T0[i] = -1.0f; T1[i] = -1.0f; T2[i] = 1.0f;
        }
        RV[i].RW = ring ? rfl(ldsi[L::HDR + 4 + 4 * i + 0]) : 1;
        RV[i].RH = ring ? rfl(ldsi[L::HDR + 4 + 4 * i + 1]) : 1;
        RV[i].rowb = ring_row_floats<STRIDE>(RV[i].RW) * 4;
        RV[i].base = lds0 + 4 * (ring ? rfl(ldsi[L::HDR + 4 + 4 * i + 2]) : L::DATA);
    }
    const float invV = 1.0f / (float)(p.n_src + 1);
    const size_t cstride_b = (p.plane_major ? plane : (size_t)D * plane) * sizeof(T);   // bytes between channels
    const size_t cl_step = p.out_cl == 2 ? plane * 16 : 16;

    // all CH/4.. channels of one quad: accumulators -> output values -> stores
    unsigned long long even_quad = 0;   // OUTCL: the packed even quad waits for the odd one (one 16-byte store per pair)
    auto finalize_store = [&](const f4& s, const f4& qq, unsigned long long& ob, int q) {
        f4 o;
        if (MODE == MODE_VARIANCE) {   // two channels per instruction; each half is the scalar sequence m = s/V, fma(qq, 1/V, -(m*m))
            const f2 iv = {invV, invV};
            const f2 ml = lo2(s) * iv, mh = hi2(s) * iv;
            o = cat2(pk_fma(lo2(qq), iv, -(ml * ml)), pk_fma(hi2(qq), iv, -(mh * mh)));
        } else if (MODE == MODE_WEIGHTED) {
            o = s * rden;
        } else {
            o = s;
        }
        if constexpr (OUTCL) {
            if ((q & 1) == 0) {
                even_quad = pack_h16x4(o);
            } else {
                store_sbase_h16x8(ob, pixo, even_quad, pack_h16x4(o));
                ob += cl_step;   // the next 8 channels: the next 16 bytes of the cell, or the next group plane (CL8)
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                store_sbase(ob, pixb, o[k]);
                ob += cstride_b;
            }
        }
    };
    auto accumulate = [&](f4& s, f4& qq, float& pair_acc, const f4& val, int q, int i) {
        if (MODE == MODE_VARIANCE) {
            const f2 vl = lo2(val), vh = hi2(val);
            s = cat2(lo2(s) + vl, hi2(s) + vh);
            qq = cat2(pk_fma(vl, vl, lo2(qq)), pk_fma(vh, vh, hi2(qq)));
        } else if (MODE == MODE_WEIGHTED) {
#pragma unroll
            for (int k = 0; k < 4; ++k) s[k] = fmaf(val[k] * r[F16 ? 0 : q][k], vw[i], s[k]);
        } else if (MODE == MODE_PAIR) {
#pragma unroll
            for (int k = 0; k < 4; ++k) pair_acc = fmaf(r[F16 ? 0 : q][k], val[k], pair_acc);
        } else {
            s = val;
        }
    };

    // ================================ main loop over steps ======================================
    const bool timing = D3D_STAMPS && a.tstats != nullptr && wave == 0;
    const bool wtiming = D3D_STAMPS && a.tstats != nullptr;  // every compute wave: its own barrier wait
    long long t_ww = 0;
    long long t_w = 0, t_w0 = 0, t_c = 0, t_mark = 0;
    if (timing) { t_mark = clock64(); if (lane == 0) atomicAdd(a.tstats + 0, (unsigned long long)(t_mark - t_start)); }
    // (s_setprio 2 / 3 on ALL compute waves: no effect, 6.49 / 6.46 ms next to 6.51 / 6.47 ms without)
    // ---- one plane of the segment (dl_ = plane index within the segment) for this wave's pixels and the current group ----
    int kx[NSRC], ky[NSRC];   // ring offset minus window origin of the current step, per view (scalar registers)
    int plan_adr = 0;   // view-major: absolute LDS byte address of the current step's plan entries
    auto load_step = [&](int k) {
        if constexpr (VIEW_MAJOR) {
            plan_adr = lds_base_bytes(lds) + 4 * (L::PLAN + (ring ? k : 0) * NSRC * 8);
            return;
        }
#pragma unroll
        for (int i = 0; i < NSRC; ++i) {
            const int* e = ldsi + L::PLAN + ((ring ? k : 0) * NSRC + i) * 8;
            kx[i] = rfl(e[6]);
            ky[i] = rfl(e[7]);
        }
    };
    auto sweep_plane = [&](const int dl_) {
            const int d = ds + dl_;
            float dv;
            if (p.depth_mode == D3D_DEPTH_PER_PIXEL) {
                float t = p.depth[(size_t)d * plane + pix];
                dv = valid ? t : 1.0f;
            } else if (p.depth_mode == D3D_DEPTH_AFFINE) {
                dv = __fadd_rn(aff_lo, __fmul_rn((float)d, aff_step));   // (no load in the plane loop)
            } else {
                dv = lds[L::PMIN + dl_];
            }
            unsigned long long ob = OUTCL ? uniform64(reinterpret_cast<unsigned short*>(p.out) +
                                                      (p.out_cl == 2 ? ((size_t)d * (p.C / 8) + c0 / 8) * plane * 8 : (size_t)d * plane * p.C + c0))
                                          : uniform64(reinterpret_cast<T*>(p.out) + (p.plane_major ? (size_t)d * p.C + c0 : (size_t)c0 * D + d) * plane);  // scalar base, once per plane
            float pair_acc = 0.0f;
            if (!valid) return;  // one EXEC region per plane instead of one branch per store

            if constexpr (VIEW_MAJOR) {
                // ---- view-major order (fp16 storage, or more than four source views) -----------------------------
                // The geometry of ONE view is live at a time (the next view's is computed while this view's taps are
                // in flight) and the accumulators of all Q chunks stay in registers until the last view: with six
                // views the chunk-major order of the fp32 / four-view path keeps 6 x (2 addresses + 4 weights) alive
                // and spills, and a scratch reload inside the plane loop waits (vmcnt) for every store in flight.
                float sa[Q][CPC], qa[Q][CPC];
#pragma unroll
                for (int q = 0; q < Q; ++q)
#pragma unroll
                    for (int k = 0; k < CPC; ++k) {
                        const float rv = F16 ? rh[F16 ? q : 0][F16 ? k : 0] : r[F16 ? 0 : q][F16 ? 0 : k];
                        sa[q][k] = (MODE == MODE_VARIANCE) ? rv : 0.0f;
                        qa[q][k] = rv * rv;
                    }
                auto accumulate_vm = [&](const float (&val)[CPC], int q, int i) {
#pragma unroll
                    for (int k = 0; k < CPC; k += 2) {
                        const f2 v = {val[k], val[k + 1]};
                        if (MODE == MODE_VARIANCE) {
                            const f2 sn = (f2){sa[q][k], sa[q][k + 1]} + v;
                            const f2 qn = pk_fma(v, v, (f2){qa[q][k], qa[q][k + 1]});
                            sa[q][k] = sn[0]; sa[q][k + 1] = sn[1];
                            qa[q][k] = qn[0]; qa[q][k + 1] = qn[1];
                        } else {   // MODE_WEIGHTED (fp32 only)
                            sa[q][k] = fmaf(v[0] * r[F16 ? 0 : q][F16 ? 0 : k], vw[i], sa[q][k]);
                            sa[q][k + 1] = fmaf(v[1] * r[F16 ? 0 : q][F16 ? 0 : k + 1], vw[i], sa[q][k + 1]);
                        }
                    }
                };
                if (ring) {
                    // Per-view constants (translation, ring size / pitch / base, the step's ring offset) come from LDS -- three
                    // broadcast reads per view and plane.  As scalar registers (17 per view, six views) most of them were spilled:
                    // 104 v_readlane + 85 s_nop in a plane loop of 1093 instructions (config 5's kernel).
                    const int vt_adr = lds0 + 4 * L::VT;
                    auto geometry = [&](int i) -> TapL {
                        typedef int i4v __attribute__((ext_vector_type(4)));
                        typedef int i2v __attribute__((ext_vector_type(2)));
                        const f4 tv = *(volatile lds_f4_ptr)(unsigned)(vt_adr + 32 * i);
                        const i4v rv = *(volatile __attribute__((address_space(3))) const i4v*)(unsigned)(vt_adr + 32 * i + 16);
                        const i2v kk = *(volatile __attribute__((address_space(3))) const i2v*)(unsigned)(plan_adr + 32 * i + 24);
                        RingView R;
                        R.RW = rv[0]; R.RH = rv[1]; R.rowb = rv[2]; R.base = rv[3];
                        return geo_ring<STRIDE>(ray[i], tv[0], tv[1], tv[2], dv, umax, vmax, kk[0], kk[1], R);
                    };
                    auto fetch = [&](const TapL& g, int q, f4 (&dst)[4]) {
                        dst[0] = lds_read4_abs(g.a0 + q * 16);
                        dst[1] = lds_read4_abs(g.a0 + q * 16 + STRIDE * 4);
                        dst[2] = lds_read4_abs(g.a1 + q * 16);
                        dst[3] = lds_read4_abs(g.a1 + q * 16 + STRIDE * 4);
                    };
                    f4 tp[2][4];
                    TapL gc = geometry(0);
                    fetch(gc, 0, tp[0]);
#pragma unroll
                    for (int i = 0; i < NSRC; ++i) {
                        // keep the scheduler from hoisting every view's geometry to the top of the plane (it would: the
                        // views are independent), which is exactly the register pressure this order avoids
                        __builtin_amdgcn_sched_barrier(0);
                        TapL gn = gc;
                        if (i + 1 < NSRC) gn = geometry(i + 1);
#pragma unroll
                        for (int q = 0; q < Q; ++q) {
                            const int u = i * Q + q;
                            if (q + 1 < Q) fetch(gc, q + 1, tp[(u + 1) & 1]);
                            else if (i + 1 < NSRC) fetch(gn, 0, tp[(u + 1) & 1]);
                            f4 (&c)[4] = tp[u & 1];
                            asm volatile("" : "+v"(c[3]));
                            float val[CPC];
                            if constexpr (F16) {
                                // same summation order as grid_sample: nw, ne, sw, se -- tap by tap ACROSS the eight channels, so that
                                // consecutive instructions are independent: the compiler puts an s_nop between an inline-asm
                                // instruction and a consumer of its result (152 of them in a loop of 1140 with the channel-major order)
                                const float tw[4] = {gc.nw, gc.ne, gc.sw, gc.se};
#pragma unroll
                                for (int k = 0; k < CPC; ++k) val[k] = 0.0f;
#pragma unroll
                                for (int tp_ = 0; tp_ < 4; ++tp_) {
#pragma unroll
                                    for (int k = 0; k < CPC; k += 2) {
                                        const int wi = k >> 1;           // word wi of a tap holds channels k (low half) and k + 1
                                        val[k] = fma_mix_lo(c[tp_][wi], tw[tp_], val[k]);
                                        val[k + 1] = fma_mix_hi(c[tp_][wi], tw[tp_], val[k + 1]);
                                    }
                                    if (tp_ < 3) __builtin_amdgcn_sched_barrier(0);   // (keep the order: the scheduler would re-chain them)
                                }
                            } else {
                                const f4 v4 = blend(c[0], c[1], c[2], c[3], gc.nw, gc.ne, gc.sw, gc.se);
#pragma unroll
                                for (int k = 0; k < CPC; ++k) val[k] = v4[k];
                            }
                            accumulate_vm(val, q, i);
                        }
                        gc = gn;
                    }
                } else {   // fallback workgroups: taps from the planar maps in global memory, one channel at a time
                    for (int i = 0; i < p.n_src; ++i) {
                        const float* __restrict__ M = p.proj34 + 12 * i;
                        const Ray rr = make_ray(M, xf, yf);
                        float u, v;
                        project(rr, M[3], M[7], M[11], dv, h, w, u, v);
                        const TapG t = make_tap_glb(u, v, h, w);
                        const T* __restrict__ gp = reinterpret_cast<const T*>(p.feats[i + 1]) + (size_t)c0 * plane + t.off;
#pragma unroll
                        for (int q = 0; q < Q; ++q) {
                            float val[CPC];
#pragma unroll
                            for (int k = 0; k < CPC; ++k) {
                                const T* __restrict__ gk = gp + (size_t)(CPC * q + k) * plane;
                                val[k] = fmaf(ldf(gk + t.dyw + t.dx), t.se, fmaf(ldf(gk + t.dyw), t.sw, fmaf(ldf(gk + t.dx), t.ne, ldf(gk) * t.nw)));
                            }
                            accumulate_vm(val, q, i);
                        }
                    }
                }
#pragma unroll
                for (int q = 0; q < Q; ++q)
#pragma unroll
                    for (int k = 0; k < CPC; ++k) {
                        float o;
                        if (MODE == MODE_VARIANCE) {
                            const float m = sa[q][k] * invV;
                            o = fmaf(qa[q][k], invV, -(m * m));
                        } else {
                            o = sa[q][k] * rden;
                        }
                        if constexpr (F16) store_sbase_h(ob, pixb, o);
                        else store_sbase(ob, pixb, o);
                        ob += cstride_b;
                    }
                return;
            }

            if (ring) {
                TapL t[NSRC];
#pragma unroll
                for (int i = 0; i < NSRC; ++i) {
                    t[i] = geo_ring<STRIDE>(ray[i], T0[i], T1[i], T2[i], dv, umax, vmax, kx[i], ky[i], RV[i]);
                }
                // Units u = (quad q, view i) in q-major order; the four taps of unit u+1 are requested
                // before unit u is blended, so LDS latency overlaps the 24 VALU ops of a unit.
                constexpr int NU = Q * NSRC;
                constexpr int PD = LDS_PIPE;  // units requested ahead of the one being blended
                f4 tp[PD + 1][4];
                auto request = [&](int u, f4 (&dst)[4]) {
                    const int q2 = u / NSRC, i2 = u % NSRC;
                    dst[0] = lds_read4_abs(t[i2].a0 + q2 * 16);
                    dst[1] = lds_read4_abs(t[i2].a0 + q2 * 16 + STRIDE * 4);
                    dst[2] = lds_read4_abs(t[i2].a1 + q2 * 16);
                    dst[3] = lds_read4_abs(t[i2].a1 + q2 * 16 + STRIDE * 4);
                };
#pragma unroll
                for (int u = 0; u < PD && u < NU; ++u) request(u, tp[u % (PD + 1)]);
                f4 s, qq;
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    const int q = u / NSRC, i = u % NSRC;
                    if (u + PD < NU) request(u + PD, tp[(u + PD) % (PD + 1)]);
                    if (i == 0) {
                        if (MODE == MODE_VARIANCE) { s = r[F16 ? 0 : q]; qq = s * s; }
                        else { s = (f4){0, 0, 0, 0}; qq = s; }
                    }
                    f4 (&c)[4] = tp[u % (PD + 1)];
                    // LDS returns in order: touching the last-requested tap first makes the compiler emit ONE
                    // s_waitcnt for the unit instead of one per tap
                    asm volatile("" : "+v"(c[3]));
                    f4 val = blend(c[0], c[1], c[2], c[3], t[i].nw, t[i].ne, t[i].sw, t[i].se);
                    accumulate(s, qq, pair_acc, val, q, i);
                    if (i == NSRC - 1 && MODE != MODE_PAIR) finalize_store(s, qq, ob, q);
                }
            } else {
                TapG t[NSRC];
#pragma unroll
                for (int i = 0; i < NSRC; ++i) {
                    float u, v;
                    project(ray[i], T0[i], T1[i], T2[i], dv, h, w, u, v);
                    t[i] = make_tap_glb(u, v, h, w);
                    if (i >= p.n_src) { t[i].nw = t[i].ne = t[i].sw = t[i].se = 0.0f; t[i].off = 0; t[i].dx = 0; t[i].dyw = 0; }
                }
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    f4 s, qq;
                    if (MODE == MODE_VARIANCE) { s = r[F16 ? 0 : q]; qq = s * s; }
                    else { s = (f4){0, 0, 0, 0}; qq = s; }
#pragma unroll
                    for (int i = 0; i < NSRC; ++i) {
                        const float* __restrict__ g = p.feats[min(i + 1, p.n_src)] + (size_t)(c0 + 4 * q) * plane + t[i].off;
                        f4 val;
#pragma unroll
                        for (int kk = 0; kk < 4; ++kk) {
                            const float* __restrict__ gk = g + (size_t)kk * plane;
                            val[kk] = fmaf(gk[t[i].dyw + t[i].dx], t[i].se,
                                           fmaf(gk[t[i].dyw], t[i].sw, fmaf(gk[t[i].dx], t[i].ne, gk[0] * t[i].nw)));
                        }
                        accumulate(s, qq, pair_acc, val, q, i);
                    }
                    if (MODE != MODE_PAIR) finalize_store(s, qq, ob, q);
                }
            }
            if (MODE == MODE_PAIR)
                store_sbase(uniform64(p.out + (size_t)d * plane), pixb, pair_acc / (float)CH);
    };
    for (int gi = 0; gi < a.ngroups; ++gi) {
        grp = gi;
        c0 = gi * CH;
        if (gi > 0) load_reference(false);   // (group 0: requested ahead of the planning)
        if (!ring) {
            // GATHER_ALL: taps straight from global memory, no windows, no steps, no barriers inside the pass: every wave of the
            // workgroup (the loader waves too) takes planes sub, sub + NW, ... of its pixel rows
            constexpr int NW = NWAVES / NPIXW;
            static_assert(NWAVES % NPIXW == 0, "the loader waves must come in whole sets of pixel waves");
            load_step(0);
            for (int dl_ = wave / NPIXW; dl_ < nplanes; dl_ += NW) sweep_plane(dl_);
            __syncthreads();   // end of the pass (uniform with the ring passes of other workgroups: one barrier per pass)
            continue;
        }
        stage(0, wave, NWAVES);  // first window of the pass: every wave of the workgroup stages (see the loaders' loop)
        for (int k = 0; k < nsteps; ++k) {
            long long ta = 0;
            if (timing) ta = clock64();
            long long tw0 = 0;
            if (wtiming) tw0 = clock64();
            __syncthreads();  // barrier k: rings hold window(k)
            if (wtiming && k > 0) t_ww += clock64() - tw0;
            if (timing) { t_mark = clock64(); t_w += t_mark - ta; if (k == 0) t_w0 = t_mark - ta; }
            load_step(k);

            for (int j = 0; sub + NSUB * j < SP; ++j) {
                const int dl_ = k * SP + sub + NSUB * j;
                if (dl_ >= nplanes) break;
                sweep_plane(dl_);
            }
            if (timing) t_c += clock64() - t_mark;
            // no loader waves (NLOADW = 0): every wave stages its share of the next step's delta once its own planes are done
            // (the delta's ring slots are not part of the window the other waves are still reading)
            if constexpr (NLOADW == 0) {
                if (k + 1 < nsteps) stage(k + 1, wave, NWAVES);
            }
        }
        __syncthreads();  // end of the pass (matches the loaders')
        if (timing) t_mark = clock64();
    }
    if (wtiming && lane == 0) atomicAdd(a.tstats + 8 + wave, (unsigned long long)t_ww);
    if (timing && lane == 0) {
        atomicAdd(a.tstats + 1, (unsigned long long)t_w);
        atomicAdd(a.tstats + 5, (unsigned long long)t_w0);  // wait for the initial window (first barrier)
        atomicAdd(a.tstats + 3, (unsigned long long)t_c);
        atomicAdd(a.tstats + 4, (unsigned long long)(clock64() - t_start));
    }
}

// ---------------------------------------------------------------------------------------------
// Channel-last copy of the source maps for the loaders: [view][group][position][CH].  A loader lane then fetches the
// CH channels of a ring position with 16-byte loads instead of CH element loads from CH different planes (the
// staging waves are bound by the number of VMEM instructions they issue, not by bytes).  One extra read + write of
// the source maps per launch (0.33 GB next to 15.7 GB of output at config 2).  The copy lives in the CALLER's
// workspace (d3d_sweep_workspace_bytes); without one the fp32 loaders read the planar maps directly.
struct PackArgs {
    const void* src[D3D_MAX_VIEWS];
};
template <int CH, typename T>
__global__ __launch_bounds__(256) void pack_channel_last_kernel(PackArgs pa, int ngroups, long plane, float* __restrict__ out) {
    // thread = (position, 16-byte chunk): consecutive lanes write the contiguous bytes of one position;
    // for a fixed channel, every Q-th lane reads consecutive positions
    constexpr int CW = CH * (int)sizeof(T) / 4, Q = CW / 4, CPC = 16 / (int)sizeof(T);
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const long pos = t / Q;
    const int q = (int)(t - pos * Q);
    if (pos >= plane) return;
    const int vg = blockIdx.y;  // view * ngroups + group
    const int v = vg / ngroups, g = vg - v * ngroups;
    const T* __restrict__ s = reinterpret_cast<const T*>(pa.src[v]) + ((size_t)g * CH + CPC * q) * plane + pos;
    f4 x;
    if (sizeof(T) == 4) {
        const float* __restrict__ sf = reinterpret_cast<const float*>(s);
        x[0] = sf[0]; x[1] = sf[plane]; x[2] = sf[2 * plane]; x[3] = sf[3 * plane];
    } else {
        const unsigned short* __restrict__ sh = reinterpret_cast<const unsigned short*>(s);
        unsigned wd[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) wd[k] = (unsigned)sh[(2 * k) * plane] | ((unsigned)sh[(2 * k + 1) * plane] << 16);
        x = __builtin_bit_cast(f4, (uint4){wd[0], wd[1], wd[2], wd[3]});
    }
    reinterpret_cast<f4*>(out + ((size_t)vg * plane + pos) * CW)[q] = x;
}

// The slots of the copy that have no view (a sweep of n_src sources runs on the template of NSRC = 2 | 4 | 6, see template_views).
// The plan puts every sample of such a slot at (-1, -1): weight 1 on the tap there and weight 0 on the other three, of which
// the last is pixel (0, 0) -- a cell the loaders stage from the slot like any other.  It only ever meets weight 0, but 0 x NaN
// is a NaN in every voxel of the patch, so the cell has to exist and hold zeros: `cells` first positions, `pitch` words apart.
__global__ void zero_first_cells_kernel(float* __restrict__ out, int cells, size_t pitch, int cw) {
    for (int i = threadIdx.x; i < cells * cw; i += blockDim.x) out[(size_t)(i / cw) * pitch + i % cw] = 0.0f;
}

// The fp32 source maps of a sweep as [view][C / 8][h * w][8] in p.workspace (for the window kernel's gather path, planesweep_window.hip)
int pack_channel_last_g8(const SweepParams& p, hipStream_t stream) {
    PackArgs pa = {};
    for (int i = 0; i < p.n_src; ++i) pa.src[i] = p.feats[i + 1];
    const long plane = (long)p.h * p.w;
    const int ngroups = p.C / 8;
    hipLaunchKernelGGL((pack_channel_last_kernel<8, float>), dim3((unsigned)ceil_div(plane * 2, 256), p.n_src * ngroups), dim3(256), 0, stream, pa,
                       ngroups, plane, reinterpret_cast<float*>(p.workspace));
    D3D_LAUNCH_CHECK("pack_channel_last_kernel launch (window gather path)");
    return D3D_OK;
}

static int group_channels(int C, int n_src, int elem_bytes);

// depth planes per workgroup segment and the number of segments (shared by the launcher and the workspace query)
static void segments(int D, long tiles, int& dseg, int& nseg) {
    int dseg_cap = DSEG_MAX;
#ifdef D3D_EXPERIMENTS
    if (const char* e = getenv("D3D_TILED_DSEG")) dseg_cap = max(DEFAULT_NSUB, min(atoi(e), DSEG_MAX));
#endif
    nseg = ceil_div(D, dseg_cap);
    // enough workgroups to fill 256 CUs a few times over; 128-plane segments measured best on config 2 (rings sized
    // per segment follow the depth-dependent window size; shorter segments pay the planning prologue more often)
    while (tiles * nseg < 4096 && nseg * 2 <= ceil_div(D, 32)) nseg *= 2;
    dseg = ceil_div(D, nseg);
    nseg = ceil_div(D, dseg);
}

// The channel-last copy pays off when the sweep is deep: it costs 2 x (n_src*C*h*w) elements of traffic.
#ifndef D3D_CL_MIN_PLANES
#define D3D_CL_MIN_PLANES 96
#endif
static bool wants_channel_last(int D, int elem_bytes) { return elem_bytes == 2 || D >= D3D_CL_MIN_PLANES; }

// the aggregation templates exist for 2, 4 and 6 source views (launch_tiled): the one that serves n_src of them
static int template_views(int n_src) { return n_src <= 2 ? 2 : n_src <= 4 ? 4 : 6; }

// One slot per view of the template, not per source: see zero_first_cells_kernel.  (The query does not know the mode; the
// one-source templates of the warp and the pair pass use the first of two slots.)
size_t tiled_workspace_bytes(int n_src, int C, int D, int h, int w, int elem_bytes) {
    if (C % 8 != 0 || n_src > 6 || n_src < 1 || !wants_channel_last(D, elem_bytes)) return 0;
    return (size_t)template_views(n_src) * C * h * w * elem_bytes;
}

#ifndef D3D_SHALLOW_PLANES
#define D3D_SHALLOW_PLANES 16   // sweeps of at most this many planes take the 32 x 8-pixel patches (0: never)
#endif
// shallow form: 32 x 8-pixel patches (4 pixel waves x 2 depth sub-ranges + 4 loaders, still 12 waves and all of the LDS):
// the per-workgroup planning prologue and first-window latency are paid once per 256 pixels instead of once per 128
constexpr int SHALLOW_NSUB = 2, SHALLOW_NLOADW = D3D_NLOADW, SHALLOW_NPIXW = 4, SHALLOW_PLANES = D3D_SHALLOW_PLANES;

template <int MODE, int NSRC, int CH, typename T, bool OUTCL = false, bool SHALLOW = false>
static int launch_one(const SweepParams& p, hipStream_t stream) {
    constexpr int CW = CH * (int)sizeof(T) / 4;
    using L = Lds<CW, NSRC>;
    constexpr int LDS_BYTES = 160 * 1024;
    constexpr int NSUBK = SHALLOW ? SHALLOW_NSUB : DEFAULT_NSUB, NLOADK = SHALLOW ? SHALLOW_NLOADW : DEFAULT_NLOADW;
    constexpr int NPIXK = SHALLOW ? SHALLOW_NPIXW : DEFAULT_NPIXW, THK = 2 * NPIXK;
    constexpr int THREADSK = 64 * (NPIXK * NSUBK + NLOADK);
    auto kern = sweep_tiled_kernel<MODE, NSRC, CH, T, OUTCL, NSUBK, NLOADK, NPIXK>;
    if (OUTCL && (size_t)p.h * p.w * p.C * 2 >= ((size_t)1 << 32)) return D3D_ERR_UNSUPPORTED;
    // per device and idempotent: set on every launch (no process-global "done" flag that a second GPU would miss)
    int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), LDS_BYTES);
    if (rc != D3D_OK) return rc;
    TiledArgs a;
    a.ngroups = p.C / CH;
    a.tiles_x = ceil_div(p.w, TW);
    a.tiles_y = ceil_div(p.h, THK);
    // a last column of at most TW/2 real pixels per row is swept in patches of TW/2 x 2 THK pixels: half as many workgroups there
    a.tall = (p.w % TW >= 1 && p.w % TW <= TW / 2) ? 1 : 0;
    a.cap_floats = LDS_BYTES / 4 - L::DATA;
#ifdef D3D_EXPERIMENTS
    if (const char* e = getenv("D3D_TILED_TALL")) a.tall = a.tall && atoi(e) != 0;   // A/B: 0 = wide patches in every column
#endif
    segments(p.D, (long)a.tiles_x * a.tiles_y * a.ngroups, a.dseg, a.nseg);   // (segment length: as for wide patches throughout)
    const long col_tiles = a.tall ? (long)(a.tiles_x - 1) * a.tiles_y + (a.tiles_y + 1) / 2 : (long)a.tiles_x * a.tiles_y;
    const long nblk = col_tiles * a.nseg;  // a workgroup sweeps every channel group of its patch
    if (nblk > 0x7fffffffL) return D3D_ERR_UNSUPPORTED;
    a.stats = nullptr;
    a.tstats = nullptr;
    a.cl = nullptr;
    {
        bool use_cl = wants_channel_last(p.D, (int)sizeof(T));
#ifdef D3D_EXPERIMENTS
        if (const char* e = getenv("D3D_TILED_CL")) use_cl = atoi(e) != 0;
#endif
        const size_t bytes = (size_t)NSRC * p.C * p.h * p.w * sizeof(T);
        if (use_cl && p.workspace && p.workspace_bytes >= bytes) {
            PackArgs pa = {};
            for (int i = 0; i < p.n_src; ++i) pa.src[i] = p.feats[i + 1];
            const long plane = (long)p.h * p.w;
            hipLaunchKernelGGL((pack_channel_last_kernel<CH, T>), dim3((unsigned)ceil_div(plane * (CW / 4), 256), p.n_src * a.ngroups),
                               dim3(256), 0, stream, pa, a.ngroups, plane, reinterpret_cast<float*>(p.workspace));
            D3D_LAUNCH_CHECK("pack_channel_last_kernel launch");
            if (p.n_src < NSRC) {
                hipLaunchKernelGGL(zero_first_cells_kernel, dim3(1), dim3(256), 0, stream,
                                   reinterpret_cast<float*>(p.workspace) + (size_t)p.n_src * a.ngroups * plane * CW,
                                   (NSRC - p.n_src) * a.ngroups, (size_t)plane * CW, CW);
                D3D_LAUNCH_CHECK("zero_first_cells_kernel launch");
            }
            a.cl = reinterpret_cast<const float*>(p.workspace);
        }
        // the fp16 loaders only read the channel-last copy (2-byte planar gathers would be VMEM-issue bound)
        if (sizeof(T) == 2 && !a.cl) return D3D_ERR_UNSUPPORTED;
    }
#ifdef D3D_EXPERIMENTS
    unsigned* stats_buf = nullptr;
    if (const char* e = getenv("D3D_TILED_STATS")) {  // debug only: synchronous, allocates
        (void)hipMalloc(&stats_buf, 12 * sizeof(unsigned) + 24 * sizeof(unsigned long long));
        (void)hipMemset(stats_buf, 0, 12 * sizeof(unsigned) + 24 * sizeof(unsigned long long));
        a.tstats = reinterpret_cast<unsigned long long*>(stats_buf + 12);
        // D3D_TILED_STATS=2: the cycle stamps alone.  The plan and staging counters are atomics of every wave and step on a
        // dozen words: with them the headline kernel takes 60 ms instead of 5.7 and the stamps time the atomics.
        if (atoi(e) != 2) a.stats = stats_buf;
    }
#endif
    hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(THREADSK), LDS_BYTES, stream, p, a);
    D3D_LAUNCH_CHECK("sweep_tiled_kernel launch");
#ifdef D3D_EXPERIMENTS
    a.stats = stats_buf;
    if (a.stats) {
        unsigned hs[12];
        unsigned long long ht[24];
        (void)hipMemcpy(hs, a.stats, sizeof(hs), hipMemcpyDeviceToHost);
        (void)hipMemcpy(ht, a.tstats, sizeof(ht), hipMemcpyDeviceToHost);
        fprintf(stderr, "[d3d tiled timing] per-WG mean cycles: compute wave 0: prologue %.0f | barrier wait %.0f (initial window %.0f) | compute %.0f | total %.0f || loader 0: barrier wait %.0f | decode+issue %.0f | wait+write %.0f\n",
                ht[0] / (double)nblk, ht[1] / (double)nblk, ht[5] / (double)nblk, ht[3] / (double)nblk, ht[4] / (double)nblk,
                ht[2] / (double)nblk, ht[6] / (double)nblk, ht[7] / (double)nblk);
        fprintf(stderr, "[d3d tiled timing] prologue phases: depth range %.0f | candidate windows %.0f | plan tables %.0f (rest: per-lane constants)\n",
                ht[16] / (double)nblk, ht[17] / (double)nblk, ht[18] / (double)nblk);
        fprintf(stderr, "[d3d tiled timing] barrier wait after the first, per compute wave (pixel rows, depth sub-range):");
        for (int wv = 0; wv < NPIXK * NSUBK; ++wv) fprintf(stderr, " %.0f", ht[8 + wv] / (double)nblk);
        fprintf(stderr, "\n");
        fprintf(stderr, "[d3d tiled stats] CH=%d elem=%d wgs=%ld ring=%u fallback=%u mean_step_planes=%.2f mean_steps=%.2f mean_ring_positions=%.0f (cap %d) dseg=%d\n",
                CH, (int)sizeof(T), nblk, hs[0], hs[1], hs[2] / (double)nblk, hs[3] / (double)nblk, hs[0] ? hs[4] / (double)hs[0] : 0.0,
                a.cap_floats / L::STRIDE, a.dseg);
        fprintf(stderr, "[d3d tiled stats] staging items per workgroup (all channel groups): %.1f | inside one rectangle %.1f (inside the image %.1f, clear of ring column 0 and row 0 %.1f, both %.1f) | slots with no item left %.1f\n",
                hs[5] / (double)nblk, hs[6] / (double)nblk, hs[8] / (double)nblk, hs[9] / (double)nblk, hs[7] / (double)nblk, hs[10] / (double)nblk);
        (void)hipFree(a.stats);
    }
#endif
    return D3D_OK;
}

static int group_channels(int C, int n_src, int elem_bytes) {
    // channels per workgroup pass.  Six fp32 rings only fit LDS with 8-channel positions; fp16 cells take 16.
    int cg = (n_src > 4 && elem_bytes == 4) ? 8 : (C >= 16 ? 16 : C);
#ifdef D3D_EXPERIMENTS
    if (const char* e = getenv("D3D_TILED_CG")) cg = atoi(e);   // must divide C
#endif
    if (cg != 8 && cg != 16 && cg != 32) cg = 8;
    while (C % cg) cg >>= 1;
    return cg;
}

template <int MODE, int NSRC>
static int launch_ch(const SweepParams& p, hipStream_t stream) {
    const int cg = (MODE == MODE_PAIR) ? p.C : group_channels(p.C, p.n_src, 4);
    // shallow sweeps of 8-channel groups (the full-resolution cascade stage, 8 planes): 32 x 8-pixel patches (see SHALLOW_*).
    // (A first attempt, 6-wave workgroups on half the LDS so that two share a CU, helped the weighted mode on the bench
    // scene but fell back to gathering inside AdaMVS views, whose windows need more than half the LDS.)
    bool shallow = p.D <= SHALLOW_PLANES && cg == 8;
#ifdef D3D_EXPERIMENTS
    if (const char* e = getenv("D3D_TILED_SHALLOW")) shallow = shallow && atoi(e) != 0;
#endif
    if constexpr (MODE == MODE_VARIANCE) {
        if (p.out_cl) {
            if constexpr (SHALLOW_PLANES > 0) {
                if (shallow) return launch_one<MODE, NSRC, 8, float, true, true>(p, stream);
            }
            switch (cg) {
                case 16: return launch_one<MODE, NSRC, 16, float, true>(p, stream);
                case 8: return launch_one<MODE, NSRC, 8, float, true>(p, stream);
            }
            return D3D_ERR_UNSUPPORTED;
        }
    }
    if (p.out_cl) return D3D_ERR_UNSUPPORTED;
    if constexpr (SHALLOW_PLANES > 0 && (MODE == MODE_VARIANCE || MODE == MODE_WEIGHTED)) {
        if (shallow) return launch_one<MODE, NSRC, 8, float, false, true>(p, stream);
    }
    switch (cg) {
        case 32: return launch_one<MODE, NSRC, 32, float>(p, stream);
        case 16: return launch_one<MODE, NSRC, 16, float>(p, stream);
        case 8: return launch_one<MODE, NSRC, 8, float>(p, stream);
    }
    return D3D_ERR_UNSUPPORTED;
}

// fp16 storage (BASELINE config 5): 16-channel groups of 32-byte cells
template <int NSRC>
static int launch_f16(const SweepParams& p, hipStream_t stream) {
    if (p.C % 16 != 0) return D3D_ERR_UNSUPPORTED;
    return launch_one<MODE_VARIANCE, NSRC, 16, __half>(p, stream);
}

// Non-default compile-time knobs of this translation unit (d3d_build_flags): empty for the production build.  The
// timing-only experiments of rounds 1-3 (no stores / no staging / no taps / no blend / no barriers: results wrong by
// construction) are gone from the source; their numbers live in profiles/r03_ab_variants.txt.
const char* tiled_build_flags() {
    return ""
#ifdef D3D_EXPERIMENTS
           " D3D_EXPERIMENTS"
#endif
#ifdef D3D_DEV_ONLY_HEADLINE
           " D3D_DEV_ONLY_HEADLINE"
#endif
#if D3D_NSUB != 4
           " D3D_NSUB"
#endif
#if D3D_NLOADW != 4
           " D3D_NLOADW"
#endif
#if D3D_SHALLOW_PLANES != 16
           " D3D_SHALLOW_PLANES"
#endif
#if D3D_CL_MIN_PLANES != 96
           " D3D_CL_MIN_PLANES"
#endif
        ;
}

int launch_tiled(int mode, const SweepParams& p, hipStream_t stream) {
#ifdef D3D_DEV_ONLY_HEADLINE   // development builds (ISA inspection): instantiate the config-2 kernel alone
    return launch_one<MODE_VARIANCE, 4, 16, float>(p, stream);
#else
    if (p.C % 8 != 0 || (mode == MODE_PAIR && p.C != 32 && p.C != 16 && p.C != 8)) {
        set_error("tiled kernel unsupported: C=%d", p.C);
        return D3D_ERR_UNSUPPORTED;
    }
    if (p.n_src > 6) {
        set_error("tiled kernel unsupported: %d source views (max 6)", p.n_src);
        return D3D_ERR_UNSUPPORTED;
    }
    if (p.elem_bytes == 2) {
        if (mode != MODE_VARIANCE || p.out_cl) return D3D_ERR_UNSUPPORTED;
        if (p.n_src > 4) return launch_f16<6>(p, stream);
        return p.n_src <= 2 ? launch_f16<2>(p, stream) : launch_f16<4>(p, stream);
    }
    switch (mode) {
        case MODE_VARIANCE:
            if (p.n_src > 4) return launch_ch<MODE_VARIANCE, 6>(p, stream);  // BASELINE config 5: 7 views
            return p.n_src <= 2 ? launch_ch<MODE_VARIANCE, 2>(p, stream) : launch_ch<MODE_VARIANCE, 4>(p, stream);
        case MODE_WEIGHTED:
            if (p.n_src > 4) return launch_ch<MODE_WEIGHTED, 6>(p, stream);
            return p.n_src <= 2 ? launch_ch<MODE_WEIGHTED, 2>(p, stream) : launch_ch<MODE_WEIGHTED, 4>(p, stream);
        case MODE_PAIR: return launch_ch<MODE_PAIR, 1>(p, stream);
        case MODE_WARP: return launch_ch<MODE_WARP, 1>(p, stream);
    }
    set_error("internal: bad mode %d", mode);
    return D3D_ERR_INVALID_ARG;
#endif
}

}  // namespace d3d
