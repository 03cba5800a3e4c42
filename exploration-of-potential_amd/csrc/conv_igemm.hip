// ep24 - bf16 implicit-GEMM convolution on CDNA4 MFMA (forward and input-gradient): the generic LDS-DMA tiled kernel and
// the streaming kernel of the memory-bound 1x1 layers.  The gather-GEMM form, its argument block and the shared epilogue
// are in igemm.h; the 3x3 stride-1 layers run in conv_patch.hip (host wrappers at the bottom of this file dispatch).
//
// Tiling here: 128 x BN x 64 per workgroup of 4 waves (64-lane), v_mfma_f32_16x16x32_bf16, fp32 accumulate; two LDS stages
// filled by LDS-DMA, two workgroups per CU.  LDS rows are 128 B (64 bf16) with the 16-B chunk index XOR-ed by (row & 7).
// Output channels are relabelled inside each wave's 64-wide span (MFMA column j of n-tile t <-> channel 4j+t) so every
// lane owns 4 consecutive channels of a pixel: 8-byte packed stores, 128 B per pixel per wave.
#include <stdlib.h>
#include <type_traits>
#include <atomic>
#include "igemm.h"

using namespace ep24_igemm;

namespace {

// kernel_opts of the _ex entry points (include/ep24.h): per call, no process-wide state
constexpr int KOPT_TILED = 1, KOPT_NARROW_EPI = 2, KOPT_PER_CLASS = 4;     // bit 2: a stride-2 input gradient as one launch per parity class
constexpr int KOPT_REMOVED = 16 | 32 | 64; // bits 4 - 6: reserved, refused (the ring without a patch, its 32 x 32 x 16 consumers, its 256 x 64 tile: DESIGN.md section 4)
constexpr int KOPT_NO_DEEP = 128;          // bit 7: A/B option - no three-stage form of the tiled kernel (the 20 x 20 level runs in 64-wide two-stage tiles, as before round 4)
constexpr int KOPT_TILED256 = 256;         // bit 8: A/B option - 1x1 stride-1 layers with 128 < K <= 256 and M < 100 000 in the tiled kernel, as before the streaming
                                           // kernel's weight tile was requested in one batch (round 5: since then it wins there too, profiles/r05_xf_ab.txt)
constexpr int KOPT_NO_WREG = 512;         // bit 9: A/B option - 3x3 stride-1 layers with <= 64 channels in the tiled kernel instead of the weights-in-registers kernel (round 5)
constexpr int KOPT_PATCH8 = 8;             // bit 3: 3x3 stride-1 layers through the 8-wave lockstep halo-patch kernel instead of the loader / consumer ring

// ---------------------------------------------------------------------------------------------------------
// LDS-DMA variant for the MFMA-bound layers: tiles go HBM/L2 -> LDS with global_load_lds_dwordx4 (no VGPR
// staging, no ds_write: the VGPR->LDS store path moves only ~79 B/clk/CU and capped the register-staged
// kernel).  The DMA writes LDS linearly (wave base + lane*16), so the XOR swizzle is applied to the per-lane
// SOURCE address: LDS unit U = row*8 + pchunk is fetched from (row, pchunk ^ (row & 7)); padding taps and the
// M / N / K tails use an out-of-range buffer offset, for which the DMA writes zeros.  Two LDS stages, one barrier per K-step: the DMA of tile t+1 is
// in flight while tile t feeds the MFMAs.
// (Round 3 built this loop as a ring of 3 / 4 LDS stages with counted vmcnt waits and a raw barrier as well - bit-identical results -
// and measured it on every layer shape the kernel runs: 30 - 40 % SLOWER almost everywhere, because three 32 KB stages leave room for
// one workgroup per CU instead of two and the second workgroup hides more latency than the deeper prefetch does;
// profiles/r03_ring_ab.txt.  Removed again.)
// A second variant kept two tiles in flight WITHOUT a third stage (both stages requested up front, tile it+2 requested as soon as
// tile `it` had been read, a second barrier per step): within +-4 % of this loop on the 1x1 layers, 613 against 627 us over all of
// them, nothing in the step (22.68 against 22.78 ms) - profiles/r03_ring_ab.txt.  Removed as well.
// NSTG = 3 (round 4, BN = 128 only): three LDS stages, two tiles in flight behind a counted wait and a raw barrier - for the layers
// whose 128-wide tiles leave at most one workgroup per CU anyway (the 20 x 20 level at B = 20), where the second co-resident workgroup
// that made two stages the better choice everywhere else (round 3, profiles/r03_ring_ab.txt) does not exist.
template <int BN, bool OUT_F32, int EPI, int NSTG = 2>
__device__ __forceinline__ void igemm_dma_tile(const IgemmArgs& p, const int tile_m, const int tile_n) {
    constexpr int WN = BN / 64, WM = 4 / WN, MT = BM / WM / 16, NT = 4;
    constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, STAGE = A_BYTES + B_BYTES;
    constexpr int A_INSTR = BM * 8 / 64 / 4;             // DMA instructions per wave for the A tile (4)
    constexpr int B_INSTR = BN * 8 / 64 / 4;             // 4 or 2
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const long m0 = (long)tile_m * BM;
    const int n0 = tile_n * BN;
    const int KC = (p.K + BK - 1) / BK;
    const int n_iter = p.T * KC;

    // Addressing is hoisted out of the K loop: per lane a 32-bit byte offset per row (tap (0,0), chunk folded in)
    // and a bit mask of the taps that fall inside the image; per K-step the address is rowoff + (scalar tap /
    // chunk offset).  Loads go through buffer descriptors: an out-of-range voffset makes the DMA write zeros, which
    // is how padding taps, the M / N tails and the K tail are filled.
    const int lchunk = (lane & 7) ^ ((lane >> 3) & 7);
    const auto src_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(p.src), 0, p.src_bytes, 0x00020000);
    const auto wt_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(p.wt), 0, p.wt_bytes, 0x00020000);
    int rowoff[A_INSTR];
    unsigned vmask[A_INSTR];
    int iy0v[A_INSTR], ix0v[A_INSTR];
#pragma unroll
    for (int i = 0; i < A_INSTR; ++i) {
        const long m = m0 + (wave * A_INSTR + i) * 8 + (lane >> 3);
        const bool rv = m < p.M;
        const int mm = rv ? (int)m : 0;
        const int n = fdiv(mm, p.d_plane);
        const int rem = mm - n * (p.GH * p.GW);
        const int gy = fdiv(rem, p.d_gw), gx = rem - gy * p.GW;
        const int iy0 = gy * p.sy, ix0 = gx * p.sx;
        rowoff[i] = (int)((((long)n * p.SH * p.SW + (long)iy0 * p.SW + ix0) * p.ld_src + lchunk * 8) * 2);
        iy0v[i] = rv ? iy0 : -(1 << 20);       // a row past M fails every tap's test
        ix0v[i] = ix0;
        vmask[i] = 0u;
    }
    // taps outer (their offsets come out of the packed tables with scalar shifts: no load), rows inner; T iterations, not 16
    const unsigned long long tdy = p.tap_dy, tdx = p.tap_dx, tsl = p.tap_slot;
    for (int t = 0; t < p.T; ++t) {
        const int dy = (int)((tdy >> (4 * t)) & 15ull) - 8, dx = (int)((tdx >> (4 * t)) & 15ull) - 8;
#pragma unroll
        for (int i = 0; i < A_INSTR; ++i) {
            const int iy = iy0v[i] + dy, ix = ix0v[i] + dx;
            if (iy >= 0 && iy < p.SH && ix >= 0 && ix < p.SW) vmask[i] |= 1u << t;
        }
    }
    const int ld2 = (int)p.ld_src * 2;
    int wvoff[B_INSTR];
#pragma unroll
    for (int i = 0; i < B_INSTR; ++i) {
        const int q = (wave * B_INSTR + i) * 8 + (lane >> 3);
        const int r = (q & ~63) + ((q & 15) << 2) + ((q >> 4) & 3);
        wvoff[i] = n0 + r < p.N ? (int)((((long)(n0 + r) * p.WT * p.K) + lchunk * 8) * 2) : OOB;
    }
    const int kmax = (p.K - lchunk * 8 + BK - 1) / BK;       // chunks kc < kmax hold real channels for this lane
    const int ktail = (p.K & (BK - 1)) ? KC - 1 : KC;        // chunks >= ktail need that per-lane check (K not a multiple of 64)

    int is_t = 0, is_kc = 0;                                 // (tap, channel chunk) of the next tile to issue
    auto issue = [&](int buf) {
        // channel-chunk outer, tap inner: the 9 taps of a chunk re-read the same ~27 KB window (L1 / L2 hits).
        // The offsets are selected with bit operations: written as `cond ? offset : OOB` the compiler emitted a divergent
        // branch around every DMA (two DMA instructions, exec masking, ~90 scalar instructions per K step).
        const int t = is_t, kc = is_kc;
        if (++is_t == p.T) { is_t = 0; ++is_kc; }
        const bool tail = kc >= ktail;                       // wave-uniform, false for every layer of the YOLOX-l path
        const int ktm = tail ? -(int)(kc < kmax) : -1;
        const int dy = (int)((tdy >> (4 * t)) & 15ull) - 8, dx = (int)((tdx >> (4 * t)) & 15ull) - 8;
        const int a_s = (dy * p.SW + dx) * ld2 + kc * (BK * 2);                   // = p.toff[t] + ...: scalar arithmetic, no table load
        const unsigned b_s = (unsigned)(((int)((tsl >> (4 * t)) & 15ull) * p.K + kc * BK) * 2);
        char* stage = smem + buf * STAGE;
#pragma unroll
        for (int i = 0; i < A_INSTR; ++i) {
            const int m = -(int)((vmask[i] >> t) & 1u) & ktm;                     // all ones: the tap is inside the image for this row
            const int vo = ((rowoff[i] + a_s) & m) | (OOB & ~m);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(src_rsrc, (lptr_t)(stage + (wave * A_INSTR + i) * 1024), 16, vo, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < B_INSTR; ++i) {
            // rows beyond N carry OOB: adding the tile offset keeps them beyond every extent (unsigned, < 2^32)
            const int v = (int)((unsigned)wvoff[i] + b_s);
            const int vo = (v & ktm) | (OOB & ~ktm);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wt_rsrc, (lptr_t)(stage + A_BYTES + (wave * B_INSTR + i) * 1024), 16, vo, 0, 0, 0);
        }
    };

    f32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int q = 0; q < NT; ++q) acc[i][q] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int frow = lane & 15, fq = lane >> 4;

    auto compute = [&](const char* la) {
        const char* lb = la + A_BYTES;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 fa[MT], fb[NT];
#pragma unroll
            for (int i = 0; i < MT; ++i)
                fa[i] = *reinterpret_cast<const bf16x8*>(la + swz(wm * (MT * 16) + i * 16 + frow, ks * 4 + fq));
#pragma unroll
            for (int q = 0; q < NT; ++q)
                fb[q] = *reinterpret_cast<const bf16x8*>(lb + swz(wn * 64 + q * 16 + frow, ks * 4 + fq));
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int q = 0; q < NT; ++q)
                    acc[i][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[q], acc[i][q], 0, 0, 0);
        }
    };
    if constexpr (NSTG >= 3) {
        // NSTG - 1 tiles in flight: before tile `it` is read this wave's DMAs of it have landed (the younger tiles may stay in flight),
        // then everybody's (barrier) - which also says that every wave is through with tile it - 1, whose stage tile it + NSTG - 1 takes
#pragma unroll
        for (int i = 0; i < NSTG - 1; ++i)
            if (i < n_iter) issue(i);
        int st = 0;                                          // stage of tile `it`
        for (int it = 0; it < n_iter; ++it) {
            const int ahead = n_iter - 1 - it;               // tiles issued behind this one
            if (NSTG >= 4 && ahead >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (A_INSTR + B_INSTR)) : "memory");
            else if (ahead >= 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A_INSTR + B_INSTR) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if (it + NSTG - 1 < n_iter) issue(st == 0 ? NSTG - 1 : st - 1);
            compute(smem + st * STAGE);
            st = st == NSTG - 1 ? 0 : st + 1;
        }
    } else {
    issue(0);
    for (int it = 0; it < n_iter; ++it) {
        __syncthreads();                       // vmcnt(0) + barrier: tile `it` has landed, stage (it+1)&1 is free
        if (it + 1 < n_iter) issue((it + 1) & 1);
        compute(smem + (it & 1) * STAGE);
    }
    }

    igemm_epilogue<BN, OUT_F32, MT, EPI>(p, acc, m0, n0, tile_m, smem);
}

template <int BN, bool OUT_F32, int EPI, int NSTG = 2>
__device__ __forceinline__ void igemm_dma_body(const IgemmArgs& p, const int bid, const int nwg) {
    // XCD-aware tile order: workgroups are dealt round-robin over the 8 XCDs, so give every XCD a contiguous run
    // of tiles (N fastest): the N tiles of one M tile and neighbouring M tiles share their operands in one L2
    const int xcd = bid & 7, qq = nwg >> 3, rr = nwg & 7;
    const int tile_id = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (bid >> 3);
    const int tiles_n = (p.N + BN - 1) / BN;
    const int tile_m = tile_id / tiles_n;
    igemm_dma_tile<BN, OUT_F32, EPI, NSTG>(p, tile_m, tile_id - tile_m * tiles_n);
}

template <int BN, bool OUT_F32, int EPI = 0>                // EPI: 0 training (statistics), 2 inference (bias, act, residual)
__global__ __launch_bounds__(256) void igemm_dma_kernel(const IgemmArgs p) {
    igemm_dma_body<BN, OUT_F32, EPI>(p, (int)blockIdx.x, (int)gridDim.x);
}

#ifndef EP24_DEEP_STAGES
#define EP24_DEEP_STAGES 3
#endif
template <int EPI>                                                                      // 0: with the batch statistics, 1: without (an input gradient)
__global__ __launch_bounds__(256) void igemm_dma_deep_kernel(const IgemmArgs p) {       // 128-wide tiles, three stages, bf16 training form
    igemm_dma_body<128, false, EPI, EP24_DEEP_STAGES>(p, (int)blockIdx.x, (int)gridDim.x);
}

// Up to four gather-GEMMs in ONE launch: the parity classes of a stride-2 input gradient (same M, N and K; 1, 2, 2 and 4 taps) used
// to be four dependent launches of one-round grids.  A workgroup finds its class from the tile prefix; inside a class the tile
// order is the single launch's (the XCD label of a workgroup is its index mod 8 up to a constant shift per class).
// (Round 5 measured two interleaved orders - an XCD running every class of one M tile, or of a chunk of 4 / 8 / 16 M tiles, back to
// back so that the classes share their dy rows in its L2: 10 - 17 % slower for single tiles, level for chunks.  The launch is not
// bound by re-reading dy; profiles/r05_s2_ab.txt.  Removed again.)
// Round 5: the classes of one launch differ in their taps and in the parity offset of their destination pixels, nothing else; the kernel
// takes ONE argument block and a small per-class table.  (As an array of four full blocks indexed by the run-time class, every field
// read was a scalar load at a computed address - 326 in the 128-wide kernel, 190 of them inside loops - where the single-problem kernel
// reads its arguments once at immediate offsets.)
struct IgemmMulti {
    IgemmArgs a;                                 // class 0's block; T, the packed tap tables and (dy0, dx0) are per class below
    int T[4];
    unsigned long long tap_dy[4], tap_dx[4], tap_slot[4];
    int dy0[4], dx0[4];
    int prefix[5];
    int n;
};

template <int BN>
__global__ __launch_bounds__(256) void igemm_dma_multi_kernel(const IgemmMulti q) {
    int cls = 0;
#pragma unroll
    for (int c = 1; c < 4; ++c)
        if (c < q.n && (int)blockIdx.x >= q.prefix[c]) cls = c;
    cls = __builtin_amdgcn_readfirstlane(cls);
    IgemmArgs p = q.a;                           // (fields are read where they are used: no copy is made)
    p.T = q.T[cls];
    p.tap_dy = q.tap_dy[cls]; p.tap_dx = q.tap_dx[cls]; p.tap_slot = q.tap_slot[cls];
    p.dy0 = q.dy0[cls]; p.dx0 = q.dx0[cls];
    igemm_dma_body<BN, false, 1>(p, (int)blockIdx.x - q.prefix[cls], q.prefix[cls + 1] - q.prefix[cls]);      // (input gradients: no statistics)
}

// ---------------------------------------------------------------------------------------------------------
// Streaming kernel for 1x1 stride-1 layers with K <= 256 (forward and input-gradient).  These layers are HBM
// bound (K/2 .. K FLOP per byte), and as 2-4 K-step tiles of the tiled kernels every workgroup spent its life in
// prologue / DMA round trip / epilogue.  Here the weight tile [BN][K] is loaded into LDS ONCE per workgroup and
// every wave streams its own 32-row blocks of the activation matrix straight from global memory into MFMA
// A-fragments (16 B per lane, rows are contiguous for a 1x1 conv): no staging, no barrier in the loop, the next
// block's loads are in flight while the current one is multiplied and stored, BN statistics stay in registers
// until the end.  A wave multiplies its rows with ALL BN columns of the tile (BN / 64 spans of 64).
//
// Round 3: the loop body is STRAIGHT-LINE code.  The round-2 form guarded every load with `if (k step < nks)`, every store with
// `if (row < M)` and the second block of an iteration with `if (u + 1 < units)`; hipcc branched round each of them and put an
// s_waitcnt vmcnt(0) in front of every load and before the first MFMA (it cannot count outstanding loads across those merges), so
// the "next block in flight" never was: a block cost 4 - 5 serial round trips.  Now rows / columns / K steps that do not exist
// are out-of-range buffer offsets (loads return zeros, stores are dropped, zeros add nothing to the statistics), the K-step count
// and the accumulate form are template parameters, and the waits the compiler emits are counted.
//
// GATHER (the Focus stem, round 3): the rows are not stored anywhere.  The source is the space-to-depth image [B][GH][GW][16] bf16
// (12 real channels), row m of the GEMM is the 3x3 neighbourhood of pixel m: K index = tap * 16 + channel, 144 real columns in
// 5 K steps of 32 (two taps each; the tenth tap is out of range and reads zeros).  A lane's 16-byte fragment of K step ks is half
// a pixel of tap 2 ks + fq / 2 - one load, as for a 1x1 layer, with the address of a neighbour and the padding test folded into
// the offset select.  The im2col form of rounds 1 - 2 wrote 224 bytes per pixel (459 MB at B = 20) and read them back twice
// (forward and weight gradient): 0.33 + 0.14 ms at the head of every step.  The weight tile is re-indexed on its way into LDS
// (HBM layout [Cout][tap * 12 + channel], row stride p.K).
//
// XF (round 5): the A operand is TRANSFORMED on its way from memory to the MFMA - the BatchNorm pass that would have produced it as a
// launch of its own happens here, in the registers the rows pass through anyway (this is the one conv kernel whose A operand does):
//   1 / 2  A = y = silu(bn(z)) (2: + residual row), z = p.src = the producing unit's raw output; y is stored to p.xf_out as
//          bn_act_fwd would have stored it (same expressions, same rounding: the rows the MFMAs read are the stored bf16 values)
//   3      A = dz = bn_act_bwd_apply(dy = p.src, z = p.xf_aux); dz is stored to p.xf_out for the weight gradient
//   4      the rows as they are, in the 16-row block structure of the other forms (the BNR input gradients: their epilogue's extra
//          rows and sums do not fit beside 32-row blocks - 430 - 600 bytes of scratch in the loop)
// Per-channel constants are folded from the fixed-point sums by every workgroup into LDS behind the weight tile (as the BatchNorm
// kernels' prologues do); block 0 also does those kernels' block-0 duties.  Host: N <= BN (one N tile: every row is made once).
// BNR (round 5, input-gradient forms): what the kernel stores is the dy of the unit BELOW (the previous Bottleneck's conv2, whose output
// this 1x1 conv read; with a shortcut the stored value is old + new, i.e. the complete gradient), so the two sums of that unit's
// BatchNorm backward - sum(du), sum(du * zhat), du = dy * silu'(bn(z)) - are taken from the rows while they leave, with the reduce
// kernel's expressions on the ROUNDED values it would have read; its launch (dy and z read once more, one dependent launch) goes.
// The sums' fp32 order differs from the reduce kernel's (per-lane partial sums, then the statistics fold): same values to fp32 rounding.
template <int BN, int H, int EPI, int NKS, bool ACC, bool GATHER = false, int XF = 0, bool BNR = false>      // EPI: 0 training (statistics), 1 training without statistics (input gradients), 2 inference (bias, act, residual)
__global__ __launch_bounds__(256, XF == 3 ? 3 : 2) void igemm_stream_kernel(const IgemmArgs p, int bpn) {
    // 4 waves x 32 rows per row group.  The transformed-A forms walk a wave's 32 rows as two blocks of 16 (XS = 2 sub-blocks: their
    // second source row and the constants need the registers - with 32 rows per block the loop spilled, and a scratch access in the
    // loop turns every counted wait into vmcnt(0)); the rows a lane owns and the order it adds them to the BatchNorm statistics are
    // the plain kernel's, so the statistics are bit-identical as well.
    constexpr int SP = BN / 64, NTW = SP * 4, MT = XF ? 1 : 2, XS = XF ? 2 : 1, RG = 128;
    static_assert(XF == 0 || XF == 4 || H == 1, "the transformed-A forms make one K pass");
    static_assert(!BNR || (EPI == 0 && !GATHER && XF == 4), "the fused reduce belongs to the plain input-gradient form in 16-row blocks (with the transformed-A form it doubled that form's VALU work and spilled: measured, not kept)");
    constexpr int OOB = 0x7FFFFFF0;
    constexpr bool XAUX = XF >= 2;                                            // a second source row beside p.src
    constexpr int XNC = XF == 3 ? 5 : XF == 4 ? 0 : 2;                        // constants per channel: (sc, sh) / (sc, sh, k1, k2, k3) / none (XF 4: the rows as they are)
    constexpr int XKP = H * 128;                                              // channels the K steps touch
    constexpr int XC_FLOATS = XF ? XNC * XKP : 0;                            // floats of transformed-A constants behind the weight tile
    static_assert(XF == 0 || (EPI == 0 && !GATHER), "the transformed-A forms are training forms of the plain 1x1 kernel");
    constexpr int NPAN_ = (H - 1) * 2 + (NKS + 1) / 2;                        // 64-channel weight panels in LDS (NPAN below)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 15, fq = lane >> 4;
    const int n_tiles = (p.N + BN - 1) / BN;
    // workgroup L runs on XCD L & 7: the n_tiles workgroups that walk the same rows get the same XCD (shared L2)
    const int xcd = blockIdx.x & 7, rest = blockIdx.x >> 3;
    // GATHER: an XCD takes a contiguous run of row groups per sweep, so the rows above and below (the other taps) are in its L2
    const int nt = rest % n_tiles, rb = GATHER ? xcd * (bpn >> 3) + rest / n_tiles : (rest / n_tiles) * 8 + xcd;
    const int n0 = nt * BN;

    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(p.src), 0, p.src_bytes, 0x00020000);
    const auto drsrc = __builtin_amdgcn_make_buffer_rsrc(p.dst, 0, p.dst_bytes, 0x00020000);
    const long n_groups = (p.M + RG - 1) / RG;
    const long my_groups = rb < n_groups ? (n_groups - rb + bpn - 1) / bpn : 0;
    const long units = my_groups * H * XS;                                 // (row group, K half) pairs / (row group, 16-row half) pairs

    typedef int v4i __attribute__((ext_vector_type(4)));
    typedef unsigned v2u __attribute__((ext_vector_type(2)));
    // GATHER: per lane and K step the neighbour (dy, dx) of its tap and the byte offset of that neighbour's half pixel
    int gdy[GATHER ? NKS : 1], gdx[GATHER ? NKS : 1], gof[GATHER ? NKS : 1];
    if constexpr (GATHER) {
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const int tap = 2 * ks + (fq >> 1);
            const int ty = (tap * 11) >> 5;                                 // tap / 3 for tap < 10
            gdy[ks] = tap < 9 ? ty - 1 : -(1 << 20);                        // the tenth tap fails the row test: zeros
            gdx[ks] = tap - 3 * ty - 1;
            gof[ks] = (((ty - 1) * p.GW + gdx[ks]) * 16 + (fq & 1) * 8) * 2;
        }
    }
    [[maybe_unused]] const auto xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(XAUX ? p.xf_aux : p.src), 0, XAUX ? p.xf_aux_bytes : 0u, 0x00020000);
    [[maybe_unused]] const auto orsrc = __builtin_amdgcn_make_buffer_rsrc(XF ? p.xf_out : (bf16*)p.dst, 0, XF ? p.xf_out_bytes : 0u, 0x00020000);
    [[maybe_unused]] const auto zrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(BNR ? p.bnr_z : p.src), 0, BNR ? p.bnr_z_bytes : 0u, 0x00020000);
    // every load is issued: a row past M (also every row of a unit past the last one) and a K step past K read zeros
    auto load = [&](bf16x8 (&A)[MT][NKS], [[maybe_unused]] bf16x8 (&X)[XAUX ? MT : 1][XAUX ? NKS : 1], long u) {
        const long g = rb + (u / (H * XS)) * bpn;
        const int h = (int)(u % H);
        const long r0 = g * RG + wave * 32 + (XF ? (int)((u / H) % XS) * 16 : 0);
        if constexpr (GATHER) {
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const long row = r0 + i * 16 + frow;
                const bool rv = row < p.M;
                const int mm = rv ? (int)row : 0;
                const int n = fdiv(mm, p.d_plane);
                const int rem = mm - n * (p.GH * p.GW);
                const int y = fdiv(rem, p.d_gw), x = rem - y * p.GW;
                const int base = mm * 32;
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    const bool ok = rv && (unsigned)(y + gdy[ks]) < (unsigned)p.GH && (unsigned)(x + gdx[ks]) < (unsigned)p.GW;
                    v4i t = __builtin_amdgcn_raw_buffer_load_b128(rsrc, ok ? base + gof[ks] : OOB, 0, 0);
                    A[i][ks] = __builtin_bit_cast(bf16x8, t);
                }
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const long row = r0 + i * 16 + frow;
            const int base = row < p.M ? (int)((row * p.ld_src + fq * 8 + h * 128) * 2) : OOB;
            [[maybe_unused]] const int xbase = XAUX && row < p.M ? (int)((row * p.xf_ldaux + fq * 8 + h * 128) * 2) : OOB;
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                const int vo = (h * 128 + ks * 32 + fq * 8 < p.K) ? base + ks * 64 : OOB;       // a select, not a branch
                v4i t = __builtin_amdgcn_raw_buffer_load_b128(rsrc, vo, 0, 0);
                A[i][ks] = __builtin_bit_cast(bf16x8, t);
                if constexpr (XAUX) {
                    const int xo = (h * 128 + ks * 32 + fq * 8 < p.K) ? xbase + ks * 64 : OOB;
                    v4i tx = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, xo, 0, 0);
                    X[i][ks] = __builtin_bit_cast(bf16x8, tx);
                }
            }
        }
    };

    f32x4 acc[MT][NTW];
    float s1[NTW], s2[NTW];
#pragma unroll
    for (int q = 0; q < NTW; ++q) { s1[q] = 0.f; s2[q] = 0.f; }
    constexpr bool infer = EPI == 2;                        // eval mode: y = act(acc + bias) + residual
    float ibias[infer ? NTW : 1];
    if constexpr (infer) {
#pragma unroll
        for (int q = 0; q < NTW; ++q) {
            const int c = n0 + (q >> 2) * 64 + 4 * frow + (q & 3);
            ibias[q] = c < p.N ? p.bias[c] : 0.f;
        }
    }
    // HH: which K half this block is (compile time: in the two-block loop body block 0 is half 0 and block 1 half H - 1)
    auto compute = [&](bf16x8 (&A)[MT][NKS], [[maybe_unused]] bf16x8 (&X)[XAUX ? MT : 1][XAUX ? NKS : 1], long u, auto hh) {
        constexpr int h = decltype(hh)::value;
        if constexpr (XF != 0 && XF != 4) {
            // the BatchNorm pass on the rows in flight: constants of a lane's 8 channels per K step from LDS (the 16 lanes of a
            // quarter read the same words: broadcast), rows >= M become zeros (they must add nothing to this unit's statistics)
            const float* xc = reinterpret_cast<const float*>(smem + NPAN_ * (BN * 128));
            const long g_ = rb + (u / XS) * bpn;
            const long r0_ = g_ * RG + wave * 32 + (int)(u % XS) * 16;
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                const int ch0 = h * 128 + ks * 32 + fq * 8;
                bf16x8 o_[MT];
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {            // four channels at a time: their constants are live, no more (registers)
                    f32x4 c_[XNC];
#pragma unroll
                    for (int q = 0; q < XNC; ++q) c_[q] = *reinterpret_cast<const f32x4*>(xc + q * XKP + ch0 + hf * 4);
#pragma unroll
                    for (int i = 0; i < MT; ++i) {
#pragma unroll
                        for (int jj = 0; jj < 4; ++jj) {
                            const int j = hf * 4 + jj;
                            if constexpr (XF == 3) {            // bn_bwd_apply_body's expressions
                                const float zz = (float)X[i][ks][j];
                                const float du = (float)A[i][ks][j] * act_grad(fmaf(zz, c_[0][jj], c_[1][jj]), 1);
                                o_[i][j] = (bf16)fmaf(-c_[4][jj], zz, fmaf(c_[2][jj], du, -c_[3][jj]));
                            } else {                            // bn_act_fwd_kernel's
                                const float uu = fmaf((float)A[i][ks][j], c_[0][jj], c_[1][jj]);
                                if constexpr (XF == 2) o_[i][j] = (bf16)(act_fwd(uu, 1) + (float)X[i][ks][j]);
                                else o_[i][j] = (bf16)act_fwd(uu, 1);
                            }
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < MT; ++i) {
                    const long row = r0_ + i * 16 + frow;
                    const bool ok = row < p.M;
                    const bf16x8 o = o_[i];
                    const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
                    A[i][ks] = ok ? o : zero8;
                    const int so = (ok && ch0 < p.K) ? (int)((row * p.xf_ldout + ch0) * 2) : OOB;
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4i, o), orsrc, so, 0, 0);
                }
            }
        }
        if constexpr (h == 0) {
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int q = 0; q < NTW; ++q) acc[i][q] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        // the weight fragments are re-read from LDS for every block: the laundered base keeps the compiler from hoisting all
        // 8 * BN / 16 of them out of the row loop into registers (128 VGPRs at BN = 128: it spilled to scratch)
        int wbase = 0;
        asm volatile("" : "+v"(wbase));
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const int kk = h * 4 + ks;
#pragma unroll
            for (int sp = 0; sp < SP; ++sp) {
                bf16x8 fb[4];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    fb[q] = *reinterpret_cast<const bf16x8*>(smem + wbase + (kk >> 1) * (BN * 128) + swz(sp * 64 + q * 16 + frow, (kk & 1) * 4 + fq));
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        acc[i][sp * 4 + q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[i][ks], fb[q], acc[i][sp * 4 + q], 0, 0, 0);
            }
        }
        if constexpr (h != H - 1) return;
        const long g = rb + (u / (H * XS)) * bpn;
        const long r0 = g * RG + wave * 32 + (XF ? (int)((u / H) % XS) * 16 : 0);
        if constexpr (infer) {
#pragma unroll
            for (int i = 0; i < MT; ++i) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long m = r0 + i * 16 + 4 * fq + r;
                    if (m >= p.M) continue;
#pragma unroll
                    for (int sp = 0; sp < SP; ++sp) {
                        const int c0 = n0 + sp * 64 + 4 * frow;
                        float v[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            v[q] = act_fwd(acc[i][sp * 4 + q][r] + ibias[sp * 4 + q], p.epi_act);
                            if (p.epi_res && c0 + q < p.N) v[q] += (float)p.epi_res[m * p.epi_ldres + c0 + q];
                        }
                        bf16* d = reinterpret_cast<bf16*>(p.dst) + m * p.ld_dst + c0;
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (c0 + q < p.N) d[q] = (bf16)v[q];
                    }
                }
            }
        } else {
            // 8-byte buffer stores, every one issued: the offset of a row >= M or a column group >= N is out of range (dropped).
            // N is a multiple of 4 here (the launcher checks), so a column group is all in or all out.
            auto voff = [&](int i, int r, int sp) {
                const long m = r0 + i * 16 + 4 * fq + r;
                const int c0 = n0 + sp * 64 + 4 * frow;
                return (m < p.M && c0 < p.N) ? (int)((m * p.ld_dst + c0) * 2) : OOB;
            };
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                v2u old[4][SP];
                [[maybe_unused]] v2u zb[BNR ? 4 : 1][BNR ? SP : 1];
                if constexpr (ACC) {                         // the old values of this 16-row block are requested before the first is needed
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int sp = 0; sp < SP; ++sp) old[r][sp] = __builtin_amdgcn_raw_buffer_load_b64(drsrc, voff(i, r, sp), 0, 0);
                }
                if constexpr (BNR) {                         // ... and the z rows of the unit below (a row >= M: out of range, zeros)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int sp = 0; sp < SP; ++sp) {
                            const long m = r0 + i * 16 + 4 * fq + r;
                            const int c0 = n0 + sp * 64 + 4 * frow;
                            zb[r][sp] = __builtin_amdgcn_raw_buffer_load_b64(zrsrc, (m < p.M && c0 < p.N) ? (int)((m * p.bnr_ldz + c0) * 2) : OOB, 0, 0);
                        }
                }
#pragma unroll
                for (int sp = 0; sp < SP; ++sp) {
                    [[maybe_unused]] f32x4 kb[BNR ? 4 : 1];  // the unit below's (sc, sh, invstd, mean * invstd) of this lane's four channels
                    if constexpr (BNR) {
                        const float* bc = reinterpret_cast<const float*>(smem + NPAN_ * (BN * 128)) + XC_FLOATS;
#pragma unroll
                        for (int q = 0; q < 4; ++q) kb[q] = *reinterpret_cast<const f32x4*>(bc + q * BN + sp * 64 + 4 * frow);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float v[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            v[q] = acc[i][sp * 4 + q][r];
                            // (an input gradient has no statistics: its launches take the form without them - EPI 1, round 5: the two sums
                            // were 384 of the ~600 vector instructions of a loop iteration beside 128 MFMAs, in a kernel bound by its
                            // issue slots; the sum of squares is one fused multiply-add)
                            if constexpr (EPI == 0 && XF != 3 && !BNR) { s1[sp * 4 + q] += v[q]; s2[sp * 4 + q] = fmaf(v[q], v[q], s2[sp * 4 + q]); }
                        }
                        if constexpr (ACC) {
                            const bf16x4 o = __builtin_bit_cast(bf16x4, old[r][sp]);
#pragma unroll
                            for (int q = 0; q < 4; ++q) v[q] += (float)o[q];
                        }
                        bf16x4 w;
#pragma unroll
                        for (int q = 0; q < 4; ++q) w[q] = (bf16)v[q];
                        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, w), drsrc, voff(i, r, sp), 0, 0);
                        if constexpr (BNR) {                 // bn_bwd_reduce_body's expressions on the rounded dy (s1: sum du, s2: sum du * zhat)
                            const bf16x4 zz4 = __builtin_bit_cast(bf16x4, zb[r][sp]);
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                const float zz = (float)zz4[q];
                                const float du = (float)w[q] * act_grad(fmaf(zz, kb[0][q], kb[1][q]), 1);
                                s1[sp * 4 + q] += du;
                                s2[sp * 4 + q] = fmaf(du, fmaf(zz, kb[2][q], -kb[3][q]), s2[sp * 4 + q]);
                            }
                        }
                    }
                }
            }
        }
    };

    // The first block of rows is requested BEFORE the weight tile is fetched into LDS: the two round trips overlap.
    bf16x8 A0[MT][NKS], A1[MT][NKS];
    bf16x8 X0[XAUX ? MT : 1][XAUX ? NKS : 1], X1[XAUX ? MT : 1][XAUX ? NKS : 1];
    load(A0, X0, 0);
    constexpr int NPAN = (H - 1) * 2 + (NKS + 1) / 2;       // every 64-channel panel the K steps of the loop read (zeros past K)
    static_assert(NPAN == NPAN_, "panels");
    // The weight tile [BN][K] -> LDS.  Every 16-byte chunk of a thread is REQUESTED before the first is written: as a loop of
    // "load, wait, ds_write" (what `for (u = tid; ...; u += 256) { v = ...; lds = v; }` compiles to) this was BN * NPAN / 32 serial round
    // trips to L2 at the head of every launch - 8 for a 128 x 128 tile, 16 for K = 256: most of the kernel's fixed ~8 us (round 5).
    // Buffer loads, so that a channel >= N or a chunk >= K is an out-of-range offset (zeros) instead of a branch round the load.
    // The transformed-A forms fold their per-channel constants between the request and the writes: one round trip for all of it.
    constexpr int NWT = GATHER ? 1 : BN * NPAN * 8 / 256;   // chunks per thread (BN * NPAN * 8 is a multiple of 256)
    static_assert(GATHER || NWT * 256 == BN * NPAN * 8, "weight tile chunks");
    [[maybe_unused]] v4i wv[NWT];
    if constexpr (GATHER) {
        for (int u = tid; u < BN * NPAN * 8; u += 256) {
            const int chunk = u & 7, L = (u >> 3) % BN, pan = (u >> 3) / BN;
            const int l = L & 63;
            const int ch = n0 + (L & ~63) + 4 * (l & 15) + (l >> 4);          // channel relabelling of the epilogue
            const int k = pan * 64 + chunk * 8;
            bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            // K index tap * 16 + c of the tile <- column tap * 12 + c of the weight row
            const int tap = k >> 4, c0 = k & 15;
            if (ch < p.N && tap < 9) {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (c0 + e < 12) v[e] = p.wt[(long)ch * p.K + tap * 12 + c0 + e];
            }
            *reinterpret_cast<bf16x8*>(smem + pan * (BN * 128) + swz(L, chunk)) = v;
        }
    } else {
        const auto wrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(p.wt), 0, p.wt_bytes, 0x00020000);
#pragma unroll
        for (int it = 0; it < NWT; ++it) {
            const int u = it * 256 + tid;
            const int chunk = u & 7, L = (u >> 3) % BN, pan = (u >> 3) / BN;
            const int l = L & 63;
            const int ch = n0 + (L & ~63) + 4 * (l & 15) + (l >> 4);          // channel relabelling of the epilogue
            const int k = pan * 64 + chunk * 8;
            const int wo = (ch < p.N && k < p.K) ? (int)(((long)ch * p.WT * p.K + k) * 2) : OOB;
            wv[it] = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wo, 0, 0);
        }
    }
    if constexpr (XF == 1 || XF == 2) {
        // bn_act_fwd_kernel's prologue: the producer's fixed-point statistics -> scale / shift per channel; block 0 keeps mean and
        // invstd for the backward and updates the running statistics
        float* xc = reinterpret_cast<float*>(smem + NPAN * (BN * 128));
        const int C = p.K;
        const long long* stats = p.xf_stats;
        const int reps = p.xf_reps;
        for (int c = tid; c < XKP; c += 256) {
            float s_ = 0.f, t_ = 0.f;
            if (c < C) {
                long long i1 = 0, i2 = 0;
                const float gmm = p.xf_gamma[c], bta = p.xf_beta[c];
                for (int rb_ = 0; rb_ < reps; rb_ += 8) {
                    long long a[8], b[8];
#pragma unroll
                    for (int r = 0; r < 8; ++r) {
                        const int rr_ = rb_ + r < reps ? rb_ + r : rb_;
                        a[r] = stats[(long)rr_ * 2 * C + c];
                        b[r] = stats[(long)rr_ * 2 * C + C + c];
                    }
#pragma unroll
                    for (int r = 0; r < 8; ++r) {
                        i1 += rb_ + r < reps ? a[r] : 0ll;
                        i2 += rb_ + r < reps ? b[r] : 0ll;
                    }
                }
                const float mean = from_fix(i1) / (float)p.M;
                float var = from_fix(i2) / (float)p.M - mean * mean;
                var = var < 0.f ? 0.f : var;
                const float invstd = rsqrtf(var + p.xf_eps);
                s_ = gmm * invstd;
                t_ = bta - mean * s_;
                if (blockIdx.x == 0) {
                    p.xf_save[c] = mean;
                    p.xf_save[C + c] = invstd;
                    if (p.xf_rmean) {
                        const float unb = p.M > 1 ? var * (float)p.M / (float)(p.M - 1) : var;
                        const float om = p.xf_rmean[c], ov = p.xf_rvar[c];
                        p.xf_rmean[c] = (1.f - p.xf_momentum) * om + p.xf_momentum * mean;
                        p.xf_rvar[c] = (1.f - p.xf_momentum) * ov + p.xf_momentum * unb;
                    }
                }
            }
            xc[c] = s_;
            xc[XKP + c] = t_;
        }
        if (blockIdx.x == 0 && tid == 0) {
            if (p.xf_nbt) *p.xf_nbt += 1;
            if (p.xf_nbt2) *p.xf_nbt2 += 1;
        }
    }
    if constexpr (XF == 3) {
        // bn_bwd_apply_body's prologue: fold the replicas of the two sums (exact integers), derive the five constants per channel;
        // block 0 publishes the sums into the parameter gradients
        float* xc = reinterpret_cast<float*>(smem + NPAN * (BN * 128));
        const int C = p.K;
        const int reps = p.xf_reps;
        const float invM = 1.f / (float)p.M;
        for (int c = tid; c < XKP; c += 256) {
            float v_[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
            if (c < C) {
                float f_[2];
                const float mean = p.xf_save[c], inv = p.xf_save[C + c], g = p.xf_gamma[c], bt_ = p.xf_beta[c];     // requested with the sums
                long long acc_[2] = {0, 0};
                int bad_[2] = {0, 0};                        // (no short-circuit: a branch per replica word kept the two sums' loads apart)
                for (int rb_ = 0; rb_ < reps; rb_ += 8) {    // both sums' replica words of a batch are requested together
                    long long a[2][8];
#pragma unroll
                    for (int w_ = 0; w_ < 2; ++w_)
#pragma unroll
                        for (int r = 0; r < 8; ++r) a[w_][r] = (w_ ? p.xf_dbeta + c : p.xf_dgamma + c)[(long)(rb_ + r < reps ? rb_ + r : rb_) * 2 * C];
#pragma unroll
                    for (int w_ = 0; w_ < 2; ++w_)
#pragma unroll
                        for (int r = 0; r < 8; ++r) {
                            acc_[w_] += rb_ + r < reps ? a[w_][r] : 0ll;
                            bad_[w_] |= (int)fixg_bad(a[w_][r]);
                        }
                }
#pragma unroll
                for (int w_ = 0; w_ < 2; ++w_) f_[w_] = bad_[w_] ? __builtin_nanf("") : from_fix_g(acc_[w_]);
                v_[0] = g * inv; v_[1] = bt_ - mean * v_[0];
                v_[2] = g * inv;
                v_[4] = v_[2] * inv * (f_[0] * invM);
                v_[3] = v_[2] * (f_[1] * invM) - v_[4] * mean;
                if (blockIdx.x == 0 && p.xf_ggrad) {        // both old values requested before either is written
                    const float og = p.xf_ggrad[c], ob = p.xf_bgrad[c];
                    p.xf_ggrad[c] = og + f_[0]; p.xf_bgrad[c] = ob + f_[1];
                }
            }
#pragma unroll
            for (int q = 0; q < 5; ++q) xc[q * XKP + c] = v_[q];
        }
    }
    if constexpr (BNR) {
        // the unit below's constants for this N tile's channels, four arrays of BN floats: scale, shift (as its forward made them),
        // invstd, mean * invstd
        float* bc = reinterpret_cast<float*>(smem + NPAN * (BN * 128)) + XC_FLOATS;
        for (int c = tid; c < BN; c += 256) {
            const int ch = n0 + c;
            float k_[4] = {0.f, 0.f, 0.f, 0.f};
            if (ch < p.N) {
                const float mean = p.bnr_mean[ch], inv = p.bnr_invstd[ch], g = p.bnr_gamma[ch], bt = p.bnr_beta[ch];
                k_[0] = g * inv; k_[1] = bt - mean * k_[0]; k_[2] = inv; k_[3] = mean * inv;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) bc[q * BN + c] = k_[q];
        }
    }
    if constexpr (!GATHER) {
#pragma unroll
        for (int it = 0; it < NWT; ++it) {
            const int u = it * 256 + tid;
            const int chunk = u & 7, L = (u >> 3) % BN, pan = (u >> 3) / BN;
            *reinterpret_cast<v4i*>(smem + pan * (BN * 128) + swz(L, chunk)) = wv[it];
        }
    }
    __syncthreads();

    // Two blocks per iteration, nothing conditional inside: with H = 2 block 0 is the first K half and block 1 the second of the
    // same rows; with H = 1 both are whole row blocks, and when `units` is odd the last block 1 is a unit past the end - its rows
    // are >= M, so it loads zeros, stores nothing and adds zeros to the statistics.
#pragma unroll 1
    for (long u = 0; u < units; u += 2) {
        load(A1, X1, u + 1);
        compute(A0, X0, u, std::integral_constant<int, 0>{});
        load(A0, X0, u + 2);
        compute(A1, X1, u + 1, std::integral_constant<int, H - 1>{});
    }

    if ((EPI == 0 || BNR) && (BNR || p.stats)) {
        __syncthreads();
        float* red = reinterpret_cast<float*>(smem);           // [4 waves][2][BN]; the weight tile is no longer needed
#pragma unroll
        for (int q = 0; q < NTW; ++q) {
            float a = s1[q], b = s2[q];
            a += __shfl_xor(a, 16, 64); a += __shfl_xor(a, 32, 64);
            b += __shfl_xor(b, 16, 64); b += __shfl_xor(b, 32, 64);
            if (fq == 0) {
                const int c = (q >> 2) * 64 + 4 * frow + (q & 3);
                red[(wave * 2 + 0) * BN + c] = a;
                red[(wave * 2 + 1) * BN + c] = b;
            }
        }
        __syncthreads();
        [[maybe_unused]] long long* st = BNR ? nullptr : p.stats + (long)(blockIdx.x % p.stats_replicas) * 2 * p.N;
        [[maybe_unused]] const long rep = BNR ? (long)(blockIdx.x % p.bnr_reps) * p.bnr_rep_stride : 0;
        for (int i = tid; i < 2 * BN; i += 256) {
            const int which = i / BN, c = i - which * BN;
            float v = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) v += red[(r * 2 + which) * BN + c];
            if (n0 + c < p.N) {
                if constexpr (BNR)     // s1 = sum du -> the beta sum, s2 = sum du * zhat -> the gamma sum (2^-36 fixed point, as bn_act_bwd_reduce)
                    atomicAdd((unsigned long long*)((which ? p.bnr_dgamma : p.bnr_dbeta) + rep + n0 + c), (unsigned long long)to_fix_g(v));
                else
                    atomicAdd((unsigned long long*)(st + (long)which * p.N + n0 + c), (unsigned long long)to_fix(v));
            }
        }
    }
}

template <int BN, int H, int NKS, bool GATHER = false, int XF = 0, bool BNR = false>
void launch_stream(const IgemmArgs& a, hipStream_t stream) {
    constexpr int RG = 128;                                    // rows per workgroup and row group, as in the kernel
    const int n_tiles = ep24_cdiv(a.N, BN);
    const long n_groups = (a.M + RG - 1) / RG;
    // ~2 workgroups per CU in total, a multiple of 8 per N tile (XCD mapping), never more than there are row groups
#ifndef EP24_STREAM_WGS
#define EP24_STREAM_WGS 512
#endif
    long bpn = (EP24_STREAM_WGS / n_tiles + 7) / 8 * 8;
    if (bpn > (n_groups + 7) / 8 * 8) bpn = (n_groups + 7) / 8 * 8;
    constexpr int NPAN = (H - 1) * 2 + (NKS + 1) / 2;          // as in the kernel: all panels its K steps touch
    // the weight tile + the per-channel constants of the transformed-A forms + the unit below's constants of the BNR forms
    size_t lds = (size_t)NPAN * BN * 128 + (size_t)(XF == 3 ? 5 * H * 128 : (XF == 1 || XF == 2) ? 2 * H * 128 : 0) * sizeof(float) + (size_t)(BNR ? 4 * BN : 0) * sizeof(float);
    if (lds < 4096) lds = 4096;                                // the statistics fold: [4 waves][2][BN] floats
    const dim3 grid((unsigned)(bpn * n_tiles));
    if constexpr (XF == 3 || BNR) {                            // input gradients: possibly a second writer of their destination
        if (a.accumulate) hipLaunchKernelGGL((igemm_stream_kernel<BN, H, 0, NKS, true, false, XF, BNR>), grid, dim3(256), lds, stream, a, (int)bpn);
        else hipLaunchKernelGGL((igemm_stream_kernel<BN, H, 0, NKS, false, false, XF, BNR>), grid, dim3(256), lds, stream, a, (int)bpn);
    } else if constexpr (XF != 0) {
        hipLaunchKernelGGL((igemm_stream_kernel<BN, H, 0, NKS, false, false, XF>), grid, dim3(256), lds, stream, a, (int)bpn);
    } else if constexpr (GATHER) {
        if (a.epi_infer) hipLaunchKernelGGL((igemm_stream_kernel<BN, H, 2, NKS, false, true>), grid, dim3(256), lds, stream, a, (int)bpn);
        else hipLaunchKernelGGL((igemm_stream_kernel<BN, H, 0, NKS, false, true>), grid, dim3(256), lds, stream, a, (int)bpn);
    } else {
        if (a.epi_infer) hipLaunchKernelGGL((igemm_stream_kernel<BN, H, 2, NKS, false>), grid, dim3(256), lds, stream, a, (int)bpn);
        else if (a.accumulate) hipLaunchKernelGGL((igemm_stream_kernel<BN, H, 1, NKS, true>), grid, dim3(256), lds, stream, a, (int)bpn);
        else if (!a.stats) hipLaunchKernelGGL((igemm_stream_kernel<BN, H, 1, NKS, false>), grid, dim3(256), lds, stream, a, (int)bpn);
        else hipLaunchKernelGGL((igemm_stream_kernel<BN, H, 0, NKS, false>), grid, dim3(256), lds, stream, a, (int)bpn);
    }
}

// the transformed-A forms (XF): which tile the plain kernel would take, N in ONE tile (every row of A is made exactly once)
template <int XF>
void launch_stream_xf(const IgemmArgs& a, hipStream_t stream) {               // K <= 128 (xf_shape_ok)
    if (a.N > 64) { if (a.K > 64) launch_stream<128, 1, 4, false, XF>(a, stream); else launch_stream<128, 1, 2, false, XF>(a, stream); }
    else          { if (a.K > 64) launch_stream<64, 1, 4, false, XF>(a, stream); else launch_stream<64, 1, 2, false, XF>(a, stream); }
}

// the plain kernel's shapes with the fused reduce (input gradients of 1x1 stride-1 convs with K <= 256): the 16-row block form (XF 4)
void launch_stream_bnr(const IgemmArgs& a, hipStream_t stream) {
    if (a.N > 64) { if (a.K > 128) launch_stream<128, 2, 4, false, 4, true>(a, stream); else if (a.K > 64) launch_stream<128, 1, 4, false, 4, true>(a, stream); else launch_stream<128, 1, 2, false, 4, true>(a, stream); }
    else          { if (a.K > 128) launch_stream<64, 2, 4, false, 4, true>(a, stream); else if (a.K > 64) launch_stream<64, 1, 4, false, 4, true>(a, stream); else launch_stream<64, 1, 2, false, 4, true>(a, stream); }
}

// Shapes the transformed-A forms take: what the plain streaming kernel takes with K <= 128 (one K pass) and N in one tile.
bool xf_shape_ok(long M, int K, int N) { return K > 0 && K % 8 == 0 && K <= 128 && N > 0 && N % 4 == 0 && N <= 128 && M > 0; }

template <int BN, bool F32>
void launch_variant(const IgemmArgs& a, unsigned tiles, hipStream_t stream) {
    constexpr size_t lds = 2 * (BM * 128 + BN * 128);
    if (a.epi_infer && !F32) hipLaunchKernelGGL((igemm_dma_kernel<BN, false, 2>), dim3(tiles), dim3(256), lds, stream, a);
    else if (!a.stats && !F32) hipLaunchKernelGGL((igemm_dma_kernel<BN, false, 1>), dim3(tiles), dim3(256), lds, stream, a);      // no batch statistics asked for: the form without the sums
    else hipLaunchKernelGGL((igemm_dma_kernel<BN, F32>), dim3(tiles), dim3(256), lds, stream, a);
}

// The kernels address their operands with 32-bit byte offsets through buffer descriptors (out-of-range = zero fill is how
// padding and tails work), so every operand extent must stay below 2 GiB and the pixel count below 2^31.
int check_extents(const IgemmArgs& a) {
    for (int t = 0; t < a.T; ++t)
        EP24_REQUIRE(a.T <= 16 && a.oy[t] >= -8 && a.oy[t] <= 7 && a.ox[t] >= -8 && a.ox[t] <= 7 && a.wslot[t] >= 0 && a.wslot[t] <= 15, EP24_E_UNSUPPORTED,
                     "conv: tap %d (offset %d, %d, weight slot %d) does not fit the packed tap tables (offsets -8 .. 7, slots 0 .. 15)", t, a.oy[t], a.ox[t], a.wslot[t]);
    const long src_b = (((long)a.B * a.SH * a.SW - 1) * a.ld_src + a.K) * 2;
    const long wt_b = (long)a.N * a.WT * a.K * 2;
    EP24_REQUIRE(src_b < 0x7FFF0000L && wt_b < 0x7FFF0000L && a.M < (1L << 31) && (long)a.B * a.SH * a.SW < (1L << 31), EP24_E_UNSUPPORTED,
                 "conv: a source of %ld bytes / weights of %ld bytes / %ld output pixels are beyond what the 32-bit tile addressing covers "
                 "(2 GiB per operand): split the batch", src_b, wt_b, (long)a.M);
    return EP24_OK;
}

// dry = true: no launch, *kernel_id receives the kernel the shape dispatches to (0 tiled, 1 halo patch, 2 streaming, 3 loader / consumer ring, 6 weights in registers; 4 and 5 are reserved and never returned)
void prepare(IgemmArgs& a, int kernel_opts) {
    a.narrow_epi = (kernel_opts & KOPT_NARROW_EPI) ? 1 : 0;
    a.src_bytes = (unsigned)((((long)a.B * a.SH * a.SW - 1) * a.ld_src + a.K) * 2);
    a.wt_bytes = (unsigned)((long)a.N * a.WT * a.K * 2);
    a.d_plane = make_fastdiv((unsigned)(a.GH * a.GW)); a.d_gw = make_fastdiv((unsigned)a.GW);
    a.tap_dy = a.tap_dx = a.tap_slot = 0ull;
    for (int t = 0; t < a.T; ++t) {
        a.toff[t] = (int)(((long)a.oy[t] * a.SW + a.ox[t]) * a.ld_src * 2);
        // (tap offsets of every conv of the path are -1 .. 1, a weight slot 0 .. 8; check_extents refuses what four bits cannot hold)
        a.tap_dy |= (unsigned long long)((a.oy[t] + 8) & 15) << (4 * t);
        a.tap_dx |= (unsigned long long)((a.ox[t] + 8) & 15) << (4 * t);
        a.tap_slot |= (unsigned long long)(a.wslot[t] & 15) << (4 * t);
    }
}

// the classes of a stride-2 input gradient as one launch of the tiled kernel (bf16 output, no bias / statistics)
int launch_multi(IgemmArgs* cls, int n, hipStream_t stream, int kernel_opts) {
    IgemmMulti q{};
    q.n = n;
    bool wide = true;
    for (int i = 0; i < n; ++i) {
        if (int rc = check_extents(cls[i])) return rc;
        prepare(cls[i], kernel_opts);
        {   // the extent of the (strided) destination for the epilogue's buffer stores (0: its pointer form)
            const IgemmArgs& c = cls[i];
            const long ext = (((long)(c.B - 1) * c.dbs + c.dp0 + (long)((c.GH - 1) * c.dsy + c.dy0) * c.DW + (c.GW - 1) * c.dsx + c.dx0) * c.ld_dst + c.N) * 2;
            cls[i].dst_bytes = (ext > 0 && ext < 0x7FFF0000L) ? (unsigned)ext : 0u;
        }
        wide = wide && cls[i].N > 64 && (long)ep24_cdiv(cls[i].M, BM) * ep24_cdiv(cls[i].N, 128) > 256;
        // one argument block for all classes: everything but the taps and the destination parity must agree
        const IgemmArgs &x = cls[i], &y = cls[0];
        EP24_REQUIRE(x.src == y.src && x.ld_src == y.ld_src && x.B == y.B && x.SH == y.SH && x.SW == y.SW && x.GH == y.GH && x.GW == y.GW && x.sy == y.sy &&
                     x.sx == y.sx && x.wt == y.wt && x.WT == y.WT && x.K == y.K && x.N == y.N && x.dst == y.dst && x.ld_dst == y.ld_dst && x.DH == y.DH &&
                     x.DW == y.DW && x.dsy == y.dsy && x.dsx == y.dsx && x.dbs == y.dbs && x.dp0 == y.dp0 && x.accumulate == y.accumulate && x.M == y.M &&
                     !x.bias && !x.stats && !x.bnr_z && !x.epi_infer, EP24_E_ARG, "conv_igemm_multi: the classes of one launch share everything but their taps and parity");
    }
    q.a = cls[0];
    for (int i = 1; i < n; ++i) q.a.dst_bytes = (q.a.dst_bytes && cls[i].dst_bytes) ? std::max(q.a.dst_bytes, cls[i].dst_bytes) : 0u;     // one descriptor over every class's pixels
    for (int i = 0; i < n; ++i) {
        q.T[i] = cls[i].T; q.tap_dy[i] = cls[i].tap_dy; q.tap_dx[i] = cls[i].tap_dx; q.tap_slot[i] = cls[i].tap_slot;
        q.dy0[i] = cls[i].dy0; q.dx0[i] = cls[i].dx0;
        q.prefix[i + 1] = q.prefix[i] + ep24_cdiv(cls[i].M, BM) * ep24_cdiv(cls[i].N, wide ? 128 : 64);
    }
    const unsigned blocks = (unsigned)q.prefix[n];
    const dim3 grid(blocks);
    if (wide) hipLaunchKernelGGL((igemm_dma_multi_kernel<128>), grid, dim3(256), 2 * (BM * 128 + 128 * 128), stream, q);
    else hipLaunchKernelGGL((igemm_dma_multi_kernel<64>), grid, dim3(256), 2 * (BM * 128 + 64 * 128), stream, q);
    EP24_LAUNCH_CHECK("ep24_conv_igemm_multi");
    return EP24_OK;
}

int launch(IgemmArgs a, bool out_f32, hipStream_t stream, int kernel_opts = 0, bool dry = false, int* kernel_id = nullptr) {
    EP24_REQUIRE(!(kernel_opts & KOPT_REMOVED), EP24_E_UNSUPPORTED,
                 "conv: kernel_opts bits 4 - 6 selected variants that were measured, lost and removed; their source is at commit 6cc7180");
    if (!dry) { if (int rc = check_extents(a)) return rc; }
    prepare(a, kernel_opts);
    const bool plain_dst = a.dsy == 1 && a.dsx == 1 && a.dy0 == 0 && a.dx0 == 0 && a.DW == a.GW && a.dp0 == 0 && a.dbs == (long)a.GH * a.GW;
    const long dst_b = ((a.M - 1) * a.ld_dst + a.N) * 2;     // the streaming kernel stores through a buffer descriptor (32-bit offsets)
    // ... and so do the 16-byte store paths of the tiled / ring epilogues where the destination's extent allows (0: their pointer form)
    const long dst_ext = plain_dst ? dst_b : (((long)(a.B - 1) * a.dbs + a.dp0 + (long)((a.GH - 1) * a.dsy + a.dy0) * a.DW + (a.GW - 1) * a.dsx + a.dx0) * a.ld_dst + a.N) * 2;
    a.dst_bytes = (!out_f32 && dst_ext > 0 && dst_ext < 0x7FFF0000L) ? (unsigned)dst_ext : 0u;
    const bool stream_ok = a.T == 1 && a.sy == 1 && a.sx == 1 && a.oy[0] == 0 && a.ox[0] == 0 && a.GH == a.SH && a.GW == a.SW &&
                           (a.K <= 128 || (a.K <= 256 && (a.M >= 100000 || !(kernel_opts & KOPT_TILED256)))) && !out_f32 && (!a.bias || a.epi_infer) && plain_dst &&
                           a.ld_dst % 4 == 0 && a.N % 4 == 0 && dst_b < 0x7FFF0000L;
    if (a.bnr_z && !stream_ok) {      // the fused BatchNorm-backward reduction lives in the 16-byte store path of the shared epilogue
        EP24_REQUIRE(plain_dst && !out_f32 && !a.accumulate && !a.narrow_epi && !a.bias && !a.epi_infer && a.N % 8 == 0 && a.ld_dst % 8 == 0 &&
                     a.bnr_ldz % 8 == 0 && ((reinterpret_cast<unsigned long long>(a.dst) | reinterpret_cast<unsigned long long>(a.bnr_z)) & 15) == 0 &&
                     a.bnr_reps > 0, EP24_E_ARG, "conv_dgrad_bnr: needs a plain, first-writer bf16 destination with channel counts / strides in multiples of 8");
    }
    if (stream_ok) {
        if (dry) { *kernel_id = 2; return EP24_OK; }
        a.dst_bytes = (unsigned)dst_b;
        if (a.bnr_z) {                 // the fused reduce of the unit below: the streaming kernel's own form of it (round 5)
            const long z_b = ((a.M - 1) * a.bnr_ldz + a.N) * 2;
            EP24_REQUIRE(!a.stats && !a.epi_infer && a.bnr_reps > 0 && a.bnr_ldz % 4 == 0 && z_b < 0x7FFF0000L && a.bnr_act == 1, EP24_E_ARG,
                         "conv_dgrad_bnr (1x1): an input gradient of a SiLU unit, z rows 8-byte aligned, operands below 2 GiB");
            a.bnr_z_bytes = (unsigned)z_b;
            launch_stream_bnr(a, stream);
            EP24_LAUNCH_CHECK("ep24_conv_igemm_stream_bnr");
            return EP24_OK;
        }
        // 128-wide tiles where N fills them (a 256-wide tile - one pass of the rows for N = 256 - needs 400 registers and a whole CU
        // per workgroup: 68 against 50 us on 80x80x256->256 with cold operands, tools/stream_ab.py)
        // K steps of 32 per K half: 2 for K <= 64, else 4 (a K tail is zero-filled on both operands)
        if (a.N > 64) { if (a.K > 128) launch_stream<128, 2, 4>(a, stream); else if (a.K > 64) launch_stream<128, 1, 4>(a, stream); else launch_stream<128, 1, 2>(a, stream); }
        else          { if (a.K > 128) launch_stream<64, 2, 4>(a, stream); else if (a.K > 64) launch_stream<64, 1, 4>(a, stream); else launch_stream<64, 1, 2>(a, stream); }
        EP24_LAUNCH_CHECK("ep24_conv_igemm_stream");
        return EP24_OK;
    }
    // 3x3 stride-1 (forward and input gradient): the halo-patch kernel, when the shape fits its LDS budget
    // (training form, or the eval-mode unit with its bias / activation / residual epilogue - the ring's 16-byte store path carries it)
    const bool infer_ring = a.epi_infer && !a.narrow_epi && (a.N & 7) == 0 && (a.ld_dst & 7) == 0 && (reinterpret_cast<unsigned long long>(a.dst) & 15) == 0 &&
                            (!a.epi_res || ((a.epi_ldres & 3) == 0 && (reinterpret_cast<unsigned long long>(a.epi_res) & 7) == 0));
    if (a.T == 9 && a.sy == 1 && a.sx == 1 && a.GH == a.SH && a.GW == a.SW && plain_dst && !out_f32 && ((!a.bias && !a.epi_infer) || infer_ring) &&
        !(kernel_opts & KOPT_TILED)) {
        int prc = EP24_OK;
        if (!a.epi_infer && !(kernel_opts & KOPT_NO_WREG) && launch_wreg(a, stream, dry, &prc)) {      // N, K <= 64: the weights live in registers
            if (dry) { *kernel_id = 6; return EP24_OK; }
            if (prc) return prc;
            EP24_LAUNCH_CHECK("ep24_conv_wreg");
            return EP24_OK;
        }
        if (!(kernel_opts & KOPT_PATCH8) && launch_ring(a, stream, dry, &prc)) {
            if (dry) { *kernel_id = 3; return EP24_OK; }
            if (prc) return prc;
            EP24_LAUNCH_CHECK("ep24_conv_ring");
            return EP24_OK;
        }
        if (!a.epi_infer && launch_patch(a, stream, dry, &prc)) {      // (the 8-wave kernel has no eval-mode epilogue)
            if (dry) { *kernel_id = 1; return EP24_OK; }
            if (prc) return prc;
            EP24_LAUNCH_CHECK("ep24_conv_patch");
            return EP24_OK;
        }
    }
    if (dry) { *kernel_id = 0; return EP24_OK; }
    // 128-wide N tiles unless that leaves at most one workgroup per CU (the 20x20 level at B = 20): 64-wide tiles then
    // double the workgroups (+3 .. +27 % on those layers)
    const bool wide = a.N > 64 && (long)ep24_cdiv(a.M, BM) * ep24_cdiv(a.N, 128) > 256;
    // ... unless the K loop is long enough for a deeper pipeline to pay: 128-wide tiles (half the A-tile traffic of two 64-wide ones),
    // one workgroup per CU, three stages
    // (forced on the layers with two workgroups per CU as well it costs +0.6 ms per step, with four stages instead of three nothing changes:
    // profiles/r04_tiled_deep_ab.txt)
    if (!wide && a.N > 64 && !out_f32 && !a.epi_infer && !(kernel_opts & KOPT_NO_DEEP) && a.T * ep24_cdiv(a.K, BK) >= 8) {
        static std::atomic<unsigned long long> done{0};
        int dev = 0;
        EP24_REQUIRE(hipGetDevice(&dev) == hipSuccess, EP24_E_LAUNCH, "conv: hipGetDevice failed");
        const unsigned long long bit = 1ull << (dev & 63);
        if (!(done.load(std::memory_order_acquire) & bit)) {
            hipError_t e = hipFuncSetAttribute((const void*)igemm_dma_deep_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            if (e == hipSuccess) e = hipFuncSetAttribute((const void*)igemm_dma_deep_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            EP24_REQUIRE(e == hipSuccess, EP24_E_LAUNCH, "conv: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed on device %d: %s", dev, hipGetErrorString(e));
            done.fetch_or(bit, std::memory_order_release);
        }
        const unsigned t128 = (unsigned)ep24_cdiv(a.M, BM) * (unsigned)ep24_cdiv(a.N, 128);
        if (a.stats) hipLaunchKernelGGL(igemm_dma_deep_kernel<0>, dim3(t128), dim3(256), EP24_DEEP_STAGES * (BM * 128 + 128 * 128), stream, a);
        else hipLaunchKernelGGL(igemm_dma_deep_kernel<1>, dim3(t128), dim3(256), EP24_DEEP_STAGES * (BM * 128 + 128 * 128), stream, a);
        EP24_LAUNCH_CHECK("ep24_conv_igemm_deep");
        return EP24_OK;
    }
    const unsigned tiles = (unsigned)ep24_cdiv(a.M, BM) * (unsigned)ep24_cdiv(a.N, wide ? 128 : 64);
    if (wide) {
        if (out_f32) launch_variant<128, true>(a, tiles, stream);
        else launch_variant<128, false>(a, tiles, stream);
    } else {
        if (out_f32) launch_variant<64, true>(a, tiles, stream);
        else launch_variant<64, false>(a, tiles, stream);
    }
    EP24_LAUNCH_CHECK("ep24_conv_igemm");
    return EP24_OK;
}

}  // namespace

static int conv_fwd_impl(const void* x, int64_t ld_x, const void* w, void* y, int64_t ld_y, int y_f32,
                         int64_t y_batch_rows, int64_t y_row0, const float* bias, int64_t* stats,
                         int stats_replicas, int B, int H, int W, int Cin, int Cout, int ksize, int stride,
                         int kernel_opts, void* stream, bool dry = false, int* kernel_id = nullptr) {
    EP24_REQUIRE(dry || (x && w && y), EP24_E_ARG, "conv_fwd: null pointer");
    EP24_REQUIRE(Cin % 8 == 0 && Cin > 0, EP24_E_ARG, "conv_fwd: Cin=%d must be a multiple of 8", Cin);
    EP24_REQUIRE((ksize == 1 || ksize == 3) && (stride == 1 || stride == 2), EP24_E_UNSUPPORTED,
                 "conv_fwd: k=%d s=%d unsupported", ksize, stride);
    EP24_REQUIRE(ld_x % 8 == 0 && (y_f32 || ld_y % 4 == 0), EP24_E_ARG, "conv_fwd: ld_x %% 8 / ld_y %% 4 alignment");
    EP24_REQUIRE(!stats || stats_replicas > 0, EP24_E_ARG, "conv_fwd: stats_replicas");
    const int pad = (ksize - 1) / 2;
    const int OH = (H + 2 * pad - ksize) / stride + 1, OW = (W + 2 * pad - ksize) / stride + 1;
    IgemmArgs a{};
    a.src = (const bf16*)x; a.ld_src = ld_x; a.B = B; a.SH = H; a.SW = W;
    a.GH = OH; a.GW = OW; a.sy = stride; a.sx = stride;
    a.T = ksize * ksize;
    for (int t = 0; t < a.T; ++t) { a.oy[t] = t / ksize - pad; a.ox[t] = t % ksize - pad; a.wslot[t] = t; }
    a.wt = (const bf16*)w; a.WT = a.T; a.K = Cin; a.N = Cout;
    a.dst = y; a.ld_dst = ld_y; a.DH = OH; a.DW = OW; a.dsy = a.dsx = 1; a.dy0 = a.dx0 = 0;
    a.dbs = y_batch_rows > 0 ? y_batch_rows : (long)OH * OW; a.dp0 = y_row0;
    a.accumulate = 0; a.bias = bias; a.stats = (long long*)stats; a.stats_replicas = stats ? stats_replicas : 1;
    a.M = (long)B * OH * OW;
    return launch(a, y_f32 != 0, (hipStream_t)stream, kernel_opts, dry, kernel_id);
}

extern "C" int ep24_conv_fwd_bf16(const void* x, int64_t ld_x, const void* w, void* y, int64_t ld_y, int y_f32,
                                  int64_t y_batch_rows, int64_t y_row0, const float* bias, int64_t* stats,
                                  int stats_replicas, int B, int H, int W, int Cin, int Cout, int ksize, int stride,
                                  void* stream) {
    return conv_fwd_impl(x, ld_x, w, y, ld_y, y_f32, y_batch_rows, y_row0, bias, stats, stats_replicas, B, H, W, Cin, Cout, ksize, stride, 0, stream);
}

extern "C" int ep24_conv_fwd_bf16_ex(const void* x, int64_t ld_x, const void* w, void* y, int64_t ld_y, int y_f32,
                                     int64_t y_batch_rows, int64_t y_row0, const float* bias, int64_t* stats,
                                     int stats_replicas, int B, int H, int W, int Cin, int Cout, int ksize, int stride,
                                     int kernel_opts, void* stream) {
    return conv_fwd_impl(x, ld_x, w, y, ld_y, y_f32, y_batch_rows, y_row0, bias, stats, stats_replicas, B, H, W, Cin, Cout, ksize, stride,
                         kernel_opts, stream);
}

// Eval-mode unit in one launch: BatchNorm's running statistics are folded into the packed weights and a bias
// (ep24_fold_bn), so conv -> BN -> act (+ residual) is the conv with y = act(acc + bias) + residual in its epilogue.
extern "C" int ep24_conv_fwd_infer_bf16(const void* x, int64_t ld_x, const void* w, const float* bias, int act, const void* res,
                                        int64_t ld_res, void* y, int64_t ld_y, int B, int H, int W, int Cin, int Cout, int ksize,
                                        int stride, void* stream) {
    EP24_REQUIRE(x && w && y && bias, EP24_E_ARG, "conv_fwd_infer: null pointer");
    EP24_REQUIRE(Cin % 8 == 0 && Cin > 0, EP24_E_ARG, "conv_fwd_infer: Cin=%d must be a multiple of 8", Cin);
    EP24_REQUIRE((ksize == 1 || ksize == 3) && (stride == 1 || stride == 2), EP24_E_UNSUPPORTED, "conv_fwd_infer: k=%d s=%d unsupported", ksize, stride);
    EP24_REQUIRE(ld_x % 8 == 0 && ld_y % 4 == 0 && (!res || ld_res % 4 == 0), EP24_E_ARG, "conv_fwd_infer: row stride alignment");
    const int pad = (ksize - 1) / 2;
    const int OH = (H + 2 * pad - ksize) / stride + 1, OW = (W + 2 * pad - ksize) / stride + 1;
    IgemmArgs a{};
    a.src = (const bf16*)x; a.ld_src = ld_x; a.B = B; a.SH = H; a.SW = W;
    a.GH = OH; a.GW = OW; a.sy = stride; a.sx = stride;
    a.T = ksize * ksize;
    for (int t = 0; t < a.T; ++t) { a.oy[t] = t / ksize - pad; a.ox[t] = t % ksize - pad; a.wslot[t] = t; }
    a.wt = (const bf16*)w; a.WT = a.T; a.K = Cin; a.N = Cout;
    a.dst = y; a.ld_dst = ld_y; a.DH = OH; a.DW = OW; a.dsy = a.dsx = 1; a.dy0 = a.dx0 = 0;
    a.dbs = (long)OH * OW; a.dp0 = 0;
    a.accumulate = 0; a.bias = bias; a.stats = nullptr; a.stats_replicas = 1;
    a.epi_infer = 1; a.epi_act = act; a.epi_res = (const bf16*)res; a.epi_ldres = ld_res;
    a.M = (long)B * OH * OW;
    return launch(a, false, (hipStream_t)stream);
}

// The Focus stem (network_blocks.py Focus: space-to-depth + BaseConv 3x3 over 12 channels) without an im2col buffer: the GATHER
// form of the streaming kernel over the space-to-depth image f16 = [B][FH][FW][16] bf16 (ep24_focus_pack); w = [Cout][ld_w] with
// column tap * 12 + channel (the packed forward copy of the [Cout][3][3][12] master, rows padded to ld_w).
static int stem_fwd_impl(const void* f16, const void* w, int64_t ld_w, const float* bias, int act, int infer, void* y, int64_t ld_y,
                         int64_t* stats, int stats_replicas, int B, int FH, int FW, int Cout, void* stream) {
    EP24_REQUIRE(f16 && w && y, EP24_E_ARG, "stem_conv_fwd: null pointer");
    EP24_REQUIRE(Cout > 0 && Cout % 4 == 0 && ld_y % 4 == 0 && ld_w >= 108, EP24_E_ARG, "stem_conv_fwd: Cout=%d ld_y=%ld ld_w=%ld", Cout, (long)ld_y, (long)ld_w);
    EP24_REQUIRE(!stats || stats_replicas > 0, EP24_E_ARG, "stem_conv_fwd: stats_replicas");
    IgemmArgs a{};
    a.src = (const bf16*)f16; a.ld_src = 16; a.B = B; a.SH = FH; a.SW = FW;
    a.GH = FH; a.GW = FW; a.sy = a.sx = 1; a.T = 1;
    a.wt = (const bf16*)w; a.WT = 1; a.K = (int)ld_w; a.N = Cout;
    a.dst = y; a.ld_dst = ld_y; a.DH = FH; a.DW = FW; a.dsy = a.dsx = 1; a.dbs = (long)FH * FW;
    a.bias = bias; a.stats = (long long*)stats; a.stats_replicas = stats ? stats_replicas : 1;
    a.epi_infer = infer; a.epi_act = act;
    a.M = (long)B * FH * FW;
    const long dst_b = ((a.M - 1) * ld_y + Cout) * 2;
    EP24_REQUIRE(a.M * 32 < 0x7FFF0000L && dst_b < 0x7FFF0000L, EP24_E_UNSUPPORTED, "stem_conv_fwd: %ld pixels are beyond the 32-bit addressing: split the batch", (long)a.M);
    prepare(a, 0);
    a.src_bytes = (unsigned)(a.M * 32);
    a.wt_bytes = (unsigned)((long)Cout * ld_w * 2);
    a.dst_bytes = (unsigned)dst_b;
    launch_stream<64, 1, 5, true>(a, (hipStream_t)stream);
    EP24_LAUNCH_CHECK("ep24_stem_conv_fwd");
    return EP24_OK;
}

extern "C" int ep24_stem_conv_fwd_bf16(const void* f16, const void* w, int64_t ld_w, void* y, int64_t ld_y, int64_t* stats,
                                       int stats_replicas, int B, int FH, int FW, int Cout, void* stream) {
    return stem_fwd_impl(f16, w, ld_w, nullptr, 0, 0, y, ld_y, stats, stats_replicas, B, FH, FW, Cout, stream);
}

extern "C" int ep24_stem_conv_fwd_infer_bf16(const void* f16, const void* w, int64_t ld_w, const float* bias, int act, void* y,
                                             int64_t ld_y, int B, int FH, int FW, int Cout, void* stream) {
    EP24_REQUIRE(bias, EP24_E_ARG, "stem_conv_fwd_infer: null bias");
    return stem_fwd_impl(f16, w, ld_w, bias, act, 1, y, ld_y, nullptr, 1, B, FH, FW, Cout, stream);
}

static int conv_dgrad_impl(const void* dy, int64_t ld_dy, const void* wt, void* dx, int64_t ld_dx,
                           int accumulate, int B, int H, int W, int Cin, int Cout_k, int ksize, int stride,
                           int kernel_opts, void* stream, bool dry = false, int* kernel_id = nullptr, const IgemmArgs* bnr = nullptr) {
    EP24_REQUIRE(dry || (dy && wt && dx), EP24_E_ARG, "conv_dgrad: null pointer");
    EP24_REQUIRE(Cout_k % 8 == 0 && Cout_k > 0, EP24_E_ARG, "conv_dgrad: Cout_k=%d must be a multiple of 8", Cout_k);
    EP24_REQUIRE((ksize == 1 || ksize == 3) && (stride == 1 || stride == 2), EP24_E_UNSUPPORTED,
                 "conv_dgrad: k=%d s=%d unsupported", ksize, stride);
    EP24_REQUIRE(ld_dy % 8 == 0 && ld_dx % 4 == 0, EP24_E_ARG, "conv_dgrad: ld alignment");
    const int pad = (ksize - 1) / 2;
    const int OH = (H + 2 * pad - ksize) / stride + 1, OW = (W + 2 * pad - ksize) / stride + 1;
    IgemmArgs a{};
    a.src = (const bf16*)dy; a.ld_src = ld_dy; a.B = B; a.SH = OH; a.SW = OW;
    a.wt = (const bf16*)wt; a.WT = ksize * ksize; a.K = Cout_k; a.N = Cin;
    a.dst = dx; a.ld_dst = ld_dx; a.DH = H; a.DW = W; a.dbs = (long)H * W; a.dp0 = 0;
    a.accumulate = accumulate; a.bias = nullptr; a.stats = nullptr; a.stats_replicas = 1;
    if (bnr) {
        a.bnr_z = bnr->bnr_z; a.bnr_ldz = bnr->bnr_ldz; a.bnr_mean = bnr->bnr_mean; a.bnr_invstd = bnr->bnr_invstd; a.bnr_gamma = bnr->bnr_gamma;
        a.bnr_beta = bnr->bnr_beta; a.bnr_dgamma = bnr->bnr_dgamma; a.bnr_dbeta = bnr->bnr_dbeta; a.bnr_rep_stride = bnr->bnr_rep_stride;
        a.bnr_reps = bnr->bnr_reps; a.bnr_act = bnr->bnr_act;
    }
    if (stride == 1) {
        // dx[y,x] = sum_{kh,kw} dy[y + pad - kh, x + pad - kw] . w[:,kh,kw,:]
        a.GH = H; a.GW = W; a.sy = a.sx = 1;
        a.T = ksize * ksize;
        for (int t = 0; t < a.T; ++t) { a.oy[t] = pad - t / ksize; a.ox[t] = pad - t % ksize; a.wslot[t] = t; }
        a.dsy = a.dsx = 1; a.dy0 = a.dx0 = 0;
        a.M = (long)B * H * W;
        return launch(a, false, (hipStream_t)stream, kernel_opts, dry, kernel_id);
    }
    if (dry) { *kernel_id = 0; return EP24_OK; }          // the parity classes of a stride-2 input gradient: the tiled kernel
    // stride 2: input pixels of parity (ph,pw) only see taps with (p + pad - k) even; one launch per class
    EP24_REQUIRE(H % 2 == 0 && W % 2 == 0, EP24_E_UNSUPPORTED, "conv_dgrad s2: odd spatial size %dx%d", H, W);
    // a 1x1 stride-2 conv reaches only the even pixels: as first writer it would leave the other three quarters of dx stale
    EP24_REQUIRE(ksize != 1 || accumulate, EP24_E_UNSUPPORTED, "conv_dgrad k=1 s=2 only accumulates (run it after another producer of dx)");
    IgemmArgs cls[4];
    int ncls = 0;
    for (int ph = 0; ph < 2; ++ph)
        for (int pw = 0; pw < 2; ++pw) {
            IgemmArgs c = a;
            c.GH = H / 2; c.GW = W / 2; c.sy = c.sx = 1;
            c.dsy = c.dsx = 2; c.dy0 = ph; c.dx0 = pw;
            c.T = 0;
            for (int kh = 0; kh < ksize; ++kh)
                for (int kw = 0; kw < ksize; ++kw) {
                    if (((ph + pad - kh) & 1) || ((pw + pad - kw) & 1)) continue;
                    // oh = (2*gy + ph + pad - kh)/2 = gy + (ph + pad - kh)/2  (exact: numerator even)
                    c.oy[c.T] = (ph + pad - kh) / 2; c.ox[c.T] = (pw + pad - kw) / 2; c.wslot[c.T] = kh * ksize + kw;
                    ++c.T;
                }
            c.M = (long)B * c.GH * c.GW;
            if (c.T == 0) continue;   // (k=1, odd parity): nothing reaches these pixels (the entry point only accumulates then)
            cls[ncls++] = c;
        }
    if (kernel_opts & KOPT_PER_CLASS) {                       // A/B: one launch per class, as before round 3
        for (int i = 0; i < ncls; ++i)
            if (int rc = launch(cls[i], false, (hipStream_t)stream, kernel_opts)) return rc;
        return EP24_OK;
    }
    return launch_multi(cls, ncls, (hipStream_t)stream, kernel_opts);
}

extern "C" int ep24_conv_dgrad_bf16(const void* dy, int64_t ld_dy, const void* wt, void* dx, int64_t ld_dx,
                                    int accumulate, int B, int H, int W, int Cin, int Cout_k, int ksize, int stride,
                                    void* stream) {
    return conv_dgrad_impl(dy, ld_dy, wt, dx, ld_dx, accumulate, B, H, W, Cin, Cout_k, ksize, stride, 0, stream);
}

extern "C" int ep24_conv_dgrad_bf16_ex(const void* dy, int64_t ld_dy, const void* wt, void* dx, int64_t ld_dx,
                                       int accumulate, int B, int H, int W, int Cin, int Cout_k, int ksize, int stride,
                                       int kernel_opts, void* stream) {
    return conv_dgrad_impl(dy, ld_dy, wt, dx, ld_dx, accumulate, B, H, W, Cin, Cout_k, ksize, stride, kernel_opts, stream);
}

// Input gradient of a stride-1 conv that is the ONLY consumer of the unit below it: dx is that unit's dy, and the epilogue takes
// the two BatchNorm-backward sums of that unit from the tile on its way out (see IgemmArgs::bnr_*).
extern "C" int ep24_conv_dgrad_bnr_bf16(const void* dy, int64_t ld_dy, const void* wt, void* dx, int64_t ld_dx, int B, int H, int W,
                                        int Cin, int Cout_k, int ksize, const void* z, int64_t ld_z, const float* mean,
                                        const float* invstd, const float* gamma, const float* beta, int64_t* dgamma, int64_t* dbeta,
                                        int64_t rep_stride, int reps, int act, void* stream) {
    EP24_REQUIRE(z && mean && invstd && gamma && beta && dgamma && dbeta, EP24_E_ARG, "conv_dgrad_bnr: null pointer");
    IgemmArgs b{};
    b.bnr_z = (const bf16*)z; b.bnr_ldz = ld_z; b.bnr_mean = mean; b.bnr_invstd = invstd; b.bnr_gamma = gamma; b.bnr_beta = beta;
    b.bnr_dgamma = (long long*)dgamma; b.bnr_dbeta = (long long*)dbeta; b.bnr_rep_stride = rep_stride; b.bnr_reps = reps; b.bnr_act = act;
    return conv_dgrad_impl(dy, ld_dy, wt, dx, ld_dx, 0, B, H, W, Cin, Cout_k, ksize, 1, 0, stream, false, nullptr, &b);
}

// ---------------------------------------------------------------------------------------------------------
// A 1x1 stride-1 conv unit together with the BatchNorm pass in front of it (igemm_stream_kernel<XF>, round 5).
extern "C" int ep24_conv1x1_xf_ok(int B, int H, int W, int Cin, int Cout) { return xf_shape_ok((long)B * H * W, Cin, Cout) ? 1 : 0; }

// Forward: y_in = silu(bn(z_in)) (+ residual) exactly as ep24_bn_act_fwd (same statistics fold, save / running statistics / counters
// by block 0), and z_out = conv1x1(y_in, w) with its batch statistics exactly as ep24_conv_fwd_bf16 - one launch.
extern "C" int ep24_conv1x1_bnin_bf16(const void* z_in, int64_t ld_zin, const int64_t* stats_in, int reps_in, const float* gamma,
                                      const float* beta, float* running_mean, float* running_var, int64_t* num_batches,
                                      int64_t* num_batches2, float* save, void* y_in, int64_t ld_yin, const void* residual,
                                      int64_t ld_res, float eps, float momentum, int act, const void* w, void* z_out, int64_t ld_zout,
                                      int64_t* stats_out, int reps_out, int B, int H, int W, int Cin, int Cout, void* stream) {
    EP24_REQUIRE(z_in && stats_in && gamma && beta && save && y_in && w && z_out, EP24_E_ARG, "conv1x1_bnin: null pointer");
    EP24_REQUIRE(act == 1, EP24_E_UNSUPPORTED, "conv1x1_bnin: SiLU units only (act = %d)", act);
    const long M = (long)B * H * W;
    EP24_REQUIRE(xf_shape_ok(M, Cin, Cout), EP24_E_UNSUPPORTED, "conv1x1_bnin: Cin=%d Cout=%d is not a shape of the transformed-A kernel (Cin, Cout <= 128)", Cin, Cout);
    EP24_REQUIRE(ld_zin % 8 == 0 && ld_yin % 8 == 0 && (!residual || ld_res % 8 == 0) && ld_zout % 4 == 0, EP24_E_ARG, "conv1x1_bnin: row stride alignment");
    EP24_REQUIRE(reps_in > 0 && (!stats_out || reps_out > 0), EP24_E_ARG, "conv1x1_bnin: replicas");
    EP24_REQUIRE(((reinterpret_cast<uintptr_t>(z_in) | reinterpret_cast<uintptr_t>(y_in) | reinterpret_cast<uintptr_t>(residual)) & 15) == 0, EP24_E_ARG,
                 "conv1x1_bnin: rows are moved 16 bytes at a time (16-byte aligned bases)");
    IgemmArgs a{};
    a.src = (const bf16*)z_in; a.ld_src = ld_zin; a.B = B; a.SH = H; a.SW = W; a.GH = H; a.GW = W; a.sy = a.sx = 1;
    a.T = 1; a.oy[0] = a.ox[0] = 0; a.wslot[0] = 0;
    a.wt = (const bf16*)w; a.WT = 1; a.K = Cin; a.N = Cout;
    a.dst = z_out; a.ld_dst = ld_zout; a.DH = H; a.DW = W; a.dsy = a.dsx = 1; a.dbs = (long)H * W;
    a.stats = (long long*)stats_out; a.stats_replicas = stats_out ? reps_out : 1;
    a.M = M;
    if (int rc = check_extents(a)) return rc;
    prepare(a, 0);
    const long dst_b = ((M - 1) * ld_zout + Cout) * 2, y_b = ((M - 1) * ld_yin + Cin) * 2, r_b = residual ? ((M - 1) * ld_res + Cin) * 2 : 0;
    EP24_REQUIRE(dst_b < 0x7FFF0000L && y_b < 0x7FFF0000L && r_b < 0x7FFF0000L, EP24_E_UNSUPPORTED, "conv1x1_bnin: an operand beyond 2 GiB: split the batch");
    a.dst_bytes = (unsigned)dst_b;
    a.xf_aux = (const bf16*)residual; a.xf_ldaux = ld_res; a.xf_aux_bytes = (unsigned)r_b;
    a.xf_out = (bf16*)y_in; a.xf_ldout = ld_yin; a.xf_out_bytes = (unsigned)y_b;
    a.xf_stats = (const long long*)stats_in; a.xf_reps = reps_in; a.xf_gamma = gamma; a.xf_beta = beta; a.xf_eps = eps; a.xf_momentum = momentum;
    a.xf_rmean = running_mean; a.xf_rvar = running_var; a.xf_nbt = (long*)num_batches; a.xf_nbt2 = (long*)num_batches2; a.xf_save = save;
    if (residual) launch_stream_xf<2>(a, (hipStream_t)stream);
    else launch_stream_xf<1>(a, (hipStream_t)stream);
    EP24_LAUNCH_CHECK("ep24_conv1x1_bnin_bf16");
    return EP24_OK;
}

// Backward: dz = ep24_bn_act_bwd_apply(dy, z, ...) (stored: the weight gradient reads it; block 0 publishes the two sums into the
// parameter gradients) and dx (+)= dz . wt as ep24_conv_dgrad_bf16 of the unit's 1x1 conv - one launch.  Cin / Cout_k as there.
extern "C" int ep24_conv1x1_dgrad_bnbwd_bf16(const void* dy, int64_t ld_dy, const void* z, int64_t ld_z, const float* save,
                                             const float* gamma, const float* beta, const int64_t* dgamma, const int64_t* dbeta,
                                             float* gamma_grad, float* beta_grad, void* dz, int64_t ld_dz, int act, int reps,
                                             const void* wt, void* dx, int64_t ld_dx, int accumulate, int B, int H, int W, int Cin,
                                             int Cout_k, void* stream) {
    EP24_REQUIRE(dy && z && save && gamma && beta && dgamma && dbeta && dz && wt && dx && reps > 0, EP24_E_ARG, "conv1x1_dgrad_bnbwd: null pointer / reps");
    EP24_REQUIRE(act == 1, EP24_E_UNSUPPORTED, "conv1x1_dgrad_bnbwd: SiLU units only (act = %d)", act);
    const long M = (long)B * H * W;
    EP24_REQUIRE(xf_shape_ok(M, Cout_k, Cin), EP24_E_UNSUPPORTED, "conv1x1_dgrad_bnbwd: Cout=%d Cin=%d is not a shape of the transformed-A kernel (both <= 128)", Cout_k, Cin);
    EP24_REQUIRE(ld_dy % 8 == 0 && ld_z % 8 == 0 && ld_dz % 8 == 0 && ld_dx % 4 == 0, EP24_E_ARG, "conv1x1_dgrad_bnbwd: row stride alignment");
    EP24_REQUIRE(((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(dz)) & 15) == 0, EP24_E_ARG,
                 "conv1x1_dgrad_bnbwd: rows are moved 16 bytes at a time (16-byte aligned bases)");
    IgemmArgs a{};
    a.src = (const bf16*)dy; a.ld_src = ld_dy; a.B = B; a.SH = H; a.SW = W; a.GH = H; a.GW = W; a.sy = a.sx = 1;
    a.T = 1; a.oy[0] = a.ox[0] = 0; a.wslot[0] = 0;
    a.wt = (const bf16*)wt; a.WT = 1; a.K = Cout_k; a.N = Cin;
    a.dst = dx; a.ld_dst = ld_dx; a.DH = H; a.DW = W; a.dsy = a.dsx = 1; a.dbs = (long)H * W;
    a.accumulate = accumulate; a.stats = nullptr; a.stats_replicas = 1;
    a.M = M;
    if (int rc = check_extents(a)) return rc;
    prepare(a, 0);
    const long dst_b = ((M - 1) * ld_dx + Cin) * 2, z_b = ((M - 1) * ld_z + Cout_k) * 2, dz_b = ((M - 1) * ld_dz + Cout_k) * 2;
    EP24_REQUIRE(dst_b < 0x7FFF0000L && z_b < 0x7FFF0000L && dz_b < 0x7FFF0000L, EP24_E_UNSUPPORTED, "conv1x1_dgrad_bnbwd: an operand beyond 2 GiB: split the batch");
    a.dst_bytes = (unsigned)dst_b;
    a.xf_aux = (const bf16*)z; a.xf_ldaux = ld_z; a.xf_aux_bytes = (unsigned)z_b;
    a.xf_out = (bf16*)dz; a.xf_ldout = ld_dz; a.xf_out_bytes = (unsigned)dz_b;
    a.xf_reps = reps; a.xf_gamma = gamma; a.xf_beta = beta; a.xf_save = const_cast<float*>(save);
    a.xf_dgamma = (const long long*)dgamma; a.xf_dbeta = (const long long*)dbeta; a.xf_ggrad = gamma_grad; a.xf_bgrad = beta_grad;
    launch_stream_xf<3>(a, (hipStream_t)stream);
    EP24_LAUNCH_CHECK("ep24_conv1x1_dgrad_bnbwd_bf16");
    return EP24_OK;
}


static int kernel_for_impl(int dgrad, int B, int H, int W, int Cin, int Cout, int ksize, int stride, int y_f32, int has_bias, int kernel_opts);

// The same for a 1x1 stride-1 conv of the streaming kernel (K <= 256), which may be a SECOND writer of dx (a Bottleneck's conv1 over a
// shortcut: what it stores, old + new, is the complete gradient of the unit below): `accumulate` as in ep24_conv_dgrad_bf16.
extern "C" int ep24_conv1x1_dgrad_bnr_bf16(const void* dy, int64_t ld_dy, const void* wt, void* dx, int64_t ld_dx, int accumulate, int B, int H, int W,
                                           int Cin, int Cout_k, const void* z, int64_t ld_z, const float* mean, const float* invstd,
                                           const float* gamma, const float* beta, int64_t* dgamma, int64_t* dbeta, int64_t rep_stride, int reps,
                                           int act, void* stream) {
    EP24_REQUIRE(z && mean && invstd && gamma && beta && dgamma && dbeta, EP24_E_ARG, "conv1x1_dgrad_bnr: null pointer");
    int kid = -1;
    if (int rc = conv_dgrad_impl(nullptr, ld_dy, nullptr, nullptr, ld_dx, accumulate, B, H, W, Cin, Cout_k, 1, 1, 0, nullptr, true, &kid)) return rc;
    EP24_REQUIRE(kid == 2, EP24_E_UNSUPPORTED, "conv1x1_dgrad_bnr: Cin=%d Cout=%d is not a layer of the streaming kernel (Cout <= 256)", Cin, Cout_k);
    IgemmArgs b{};
    b.bnr_z = (const bf16*)z; b.bnr_ldz = ld_z; b.bnr_mean = mean; b.bnr_invstd = invstd; b.bnr_gamma = gamma; b.bnr_beta = beta;
    b.bnr_dgamma = (long long*)dgamma; b.bnr_dbeta = (long long*)dbeta; b.bnr_rep_stride = rep_stride; b.bnr_reps = reps; b.bnr_act = act;
    return conv_dgrad_impl(dy, ld_dy, wt, dx, ld_dx, accumulate, B, H, W, Cin, Cout_k, 1, 1, 0, stream, false, nullptr, &b);
}

extern "C" int ep24_conv_kernel_for(int dgrad, int B, int H, int W, int Cin, int Cout, int ksize, int stride, int y_f32, int has_bias) {
    return kernel_for_impl(dgrad, B, H, W, Cin, Cout, ksize, stride, y_f32, has_bias, 0);
}

extern "C" int ep24_conv_kernel_for_ex(int dgrad, int B, int H, int W, int Cin, int Cout, int ksize, int stride, int y_f32, int has_bias,
                                       int kernel_opts) {
    return kernel_for_impl(dgrad, B, H, W, Cin, Cout, ksize, stride, y_f32, has_bias, kernel_opts);
}

static int kernel_for_impl(int dgrad, int B, int H, int W, int Cin, int Cout, int ksize, int stride, int y_f32, int has_bias, int kernel_opts) {
    int id = -1;
    const float* fake_bias = has_bias ? reinterpret_cast<const float*>(16) : nullptr;      // only tested for null
    const int c8 = (Cout + 7) / 8 * 8;
    const int rc = dgrad ? conv_dgrad_impl(nullptr, c8, nullptr, nullptr, (Cin + 3) / 4 * 4, 0, B, H, W, Cin, c8, ksize, stride, kernel_opts, nullptr, true, &id)
                         : conv_fwd_impl(nullptr, Cin, nullptr, nullptr, y_f32 ? Cout : (Cout + 3) / 4 * 4, y_f32, 0, 0, fake_bias, nullptr, 1, B, H, W, Cin, Cout,
                                         ksize, stride, kernel_opts, nullptr, true, &id);
    return rc ? rc : id;
}
