// conv0_split.hip -- conv0 (32 -> 8 channels, reference models/mvsnet.py:36, block models/module.py:26-33) for fp32
// volumes with SPLIT OPERANDS on the bf16 matrix cores: Winograd F(4,3) along z as in conv_winograd.hip, but every
// transformed activation and every transformed weight is written as the sum of three bf16 numbers
//     a = a1 + a2 + a3,   a1 = bf16(a), a2 = bf16(a - a1), a3 = bf16(a - a1 - a2)        (round to nearest even)
// and the fp32 product a * b is evaluated as the six leading cross products
//     a1 b1 + (a1 b2 + a2 b1) + (a2 b2 + a1 b3 + a3 b1)
// on v_mfma_f32_16x16x32_bf16 with fp32 accumulation.  A bf16 x bf16 product is exact in fp32; |a2| <= 2^-9 |a|,
// |a3| <= 2^-18 |a| (same for b), so the dropped terms a2 b3 + a3 b2 + a3 b3 are <= 2^-26 |a b| -- a quarter of an
// fp32 ulp of the product.  Arithmetic is therefore fp32-equivalent (not bit-equal: the MFMA adds its 32 products
// in its own order), at 16x the fp32 MFMA rate per instruction: 6 x 1/16 of the matrix-pipe time, and far less
// power than the fp32 MFMA path, which runs power-limited at ~52 % executed-MFMA utilisation.
//
// Structure (conv0_w48t_kernel): PERSISTENT blocks with PRODUCER and CONSUMER waves on a 4 (z) x 8 (y) x 32 (x) tile.
// The bf16 matrix pipe and the vector ALUs DO overlap (unlike the fp32 MFMA): in the first form of this kernel (one
// 4 x 4 x 32 tile per 4-wave block; conv0_w43s_kernel in commit c2f08ac) a wave's 432 MFMAs were 6.9 k of a tile's
// 40.7 k cycles, the rest barriers, waiting for loads, transform and split.  So the two kinds of work belong on
// different waves that run at the same time:
//   * one block per CU, 512 threads, looping over its tiles (tile index = block + j * grid: a tile keeps its XCD);
//   * waves 4-7 PRODUCE: per 8-channel chunk, raw buffer loads of the 10 x 34 halo's six input planes (one register
//     set, refilled column by column as soon as a column is transformed: the loads run two steps ahead), Winograd
//     transform in fp32, three-way bf16 split (18 VALU per 4 values: v_cvt_pk_bf16_f32, shift / mask, v_pk_add_f32),
//     ds_write_b64.  A chunk is consumed in two HALF-STEPS of three transformed planes each (a whole chunk of the
//     taller halo, 97.9 KB, does not fit twice in LDS): the producers transform a chunk once, write U0..U2 into the
//     half-0 buffer and keep U3..U5 in registers for the half-1 buffer one step later (two 49.0 KB buffers);
//   * waves 0-3 CONSUME: 108 MFMAs per half-step on the current buffer, A fragments read two (piece, unit) combos
//     ahead, the next half-step's 18 B fragments requested during the step into a second register set; the output
//     transform + stores of the previous tile run in two of the steps (own 48 KB exchange tile);
//   * ONE block barrier per half-step; nothing of a tile's prologue or epilogue is exposed except for a block's
//     first and last tile.
// Against the 4 x 4 x 32 tile of round 4 (6 x 34 halo) the taller tile loads, transforms and splits 1.33 instead of
// 1.59 halo values per output (y, x) position, and the 256 producer threads cover 680 of 768 column slots instead of
// 408 of 512.
// Selected by MVS_CONV0_SPLIT (csrc/conv3d_direct.hip); the fp32-MFMA kernels stay selectable.
#include <cstring>
#include <type_traits>

#include "mvs_internal.h"
#include "storage.h"
#include "mfma16_ops.h"

namespace mvs {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

namespace c48t {
constexpr int TZ = 4, TY = 8, TX = 32;
constexpr int HY = TY + 2, HX = TX + 2;
constexpr int NT_PLANES = 6, NPL = 3;           // transformed planes per chunk / per half-step buffer
constexpr int VOX = HY * HX;                    // 340 voxels per halo plane
constexpr int PLANE_E = VOX * 8;                // bf16 elements of one (piece, plane)
constexpr int PIECE_E = NPL * PLANE_E;          // 8,160
constexpr int BUF_E = 3 * PIECE_E;              // 24,480 elements = 48,960 B
constexpr int NCOL = VOX * 2;                   // z-columns of 4-channel pieces (y, x, half): 680
constexpr int CPT = (NCOL + 255) / 256;         // 3
constexpr int NPOS = TY * TX;                   // 256 (y, x) positions
constexpr int EXS = 8;                          // floats per position in the exchange tile (no padding: LDS is full)
constexpr int MAXT = 512;                       // tiles per block the origin table holds (the launcher sizes the grid)
static_assert(2 * BUF_E * 2 + NT_PLANES * NPOS * EXS * 4 + MAXT * 16 <= 160 * 1024, "LDS of conv0_w48t");
// B fragment bytes of half-step s = (chunk c, half h): planes 3 h .. 3 h + 2 of chunk c
constexpr unsigned bstep(int s) { return (unsigned)(((s >> 1) * NT_PLANES + 3 * (s & 1)) * 9) * 1024u; }
// chunk of step c in the block's k-th tile: odd tiles run the chunks backwards.  Each XCD's 32 blocks run their k-th
// tiles together, and 32 tiles of this size touch ~5.4 MB of input (3.2 z-tiles of the XCD's band), more than its 4 MB L2:
// the z-halo planes a tile shares with the previous round's tiles were evicted before they were read again (FETCH_SIZE
// 288 -> 342 MB against the 4 x 4 x 32 tile).  Reversed, the chunk a round ends with is the one the next begins with,
// and the reuse distance of the shared planes shrinks from a whole round to 0, 2, 4, 6 chunk-steps: 342 -> 314 MB.
__device__ __forceinline__ int chunk_of(int k, int c) { return (k & 1) ? 3 - c : c; }
__device__ __forceinline__ unsigned bofs(int chunk, int h) { return (unsigned)((chunk * NT_PLANES + 3 * h) * 9) * 1024u; }
}  // namespace c48t

// 4 fp32 values -> three 8-byte bf16 pairs (split_stage: mfma16_ops.h)
__device__ __forceinline__ void split3x(const f32x4 v, u32x2& p1, u32x2& p2, u32x2& p3) {
    unsigned a0, a1, b0, b1, c0, c1;
    const f32x2 r0 = split_stage((f32x2){v.x, v.y}, a0), r1 = split_stage((f32x2){v.z, v.w}, a1);
    const f32x2 q0 = split_stage(r0, b0), q1 = split_stage(r1, b1);
    c0 = __builtin_bit_cast(unsigned, __builtin_convertvector(q0, bf16x2));
    c1 = __builtin_bit_cast(unsigned, __builtin_convertvector(q1, bf16x2));
    p1 = (u32x2){a0, a1};
    p2 = (u32x2){b0, b1};
    p3 = (u32x2){c0, c1};
}

// One half-step of a consumer wave: 9 (A piece p, unit i) combos; a combo reads its 4 A fragments (halo rows) once for
// 6 (3 - p) MFMAs on two alternating accumulators.  Units 0 and 1 use the B fragments of the wave's first plane
// (B[0]), unit 2 those of its second (B[1]).  The A fragments are requested TWO combos ahead into a ring of three
// register sets: with a distance of one the ds_read latency under load (~250 cycles against the 96-288 cycles of a
// combo's MFMAs) was exposed at every combo.  The scheduler is held to this order (sched_barrier): left alone it hoists
// every ds_read of the unrolled step and spills.
__device__ __forceinline__ void c48t_step_mfmas(const unsigned short* __restrict__ tile, const int (&aoff)[3],
                                                const u32x4 (&B)[2][3][3], u32x4 (&Bn)[2][3][3],
                                                __amdgpu_buffer_rsrc_t brs, const unsigned (&bvoff)[2], unsigned bnext,
                                                f32x4 (&acc)[3][2]) {
    using namespace c48t;
    constexpr int NC = 9;
    u32x4 a[3][4];
    auto request = [&](int n) {
        const int pn = n / 3, in = n % 3;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            a[n % 3][j] = *reinterpret_cast<const u32x4*>(tile + pn * PIECE_E + aoff[in] + j * HX * 8);
    };
    request(0);
    request(1);
#pragma unroll
    for (int n = 0; n < NC; ++n) {
        const int p = n / 3, i = n % 3;
        if (n + 2 < NC) request(n + 2);
        // two of the NEXT step's 18 B fragments per combo: issued as one burst at the start of the step the 18 loads
        // took 1.0-2.3 k cycles to get into the CU's vector-memory queue (64 B/clk: a fragment is 16 cycles, and the
        // producers' activation loads share the queue) with the MFMAs waiting behind them
#pragma unroll
        for (int f = 2 * n; f < 2 * n + 2; ++f)
            Bn[f / 9][(f / 3) % 3][f % 3] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(
                brs, (int)bvoff[f / 9], (int)(bnext + (unsigned)(f % 9) * 1024u), 0));
        const int pl = i == 2 ? 1 : 0;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int q = 0; q < 3 - p; ++q)
#pragma unroll
                for (int rr = 0; rr < 2; ++rr)
                    acc[i][rr] = mfma16<MVS_BF16>(a[n % 3][rr + ky], B[pl][ky][q], acc[i][rr]);
        __builtin_amdgcn_sched_barrier(0);
    }
}

__global__ __launch_bounds__(512) void conv0_w48t_kernel(
    const float* __restrict__ x,             // [4][D][H][W][8] fp32
    const unsigned short* __restrict__ bp,   // [4 chunks][6 t][3 ky][3 pieces][64 lanes][8] bf16 Toeplitz panel
    const float* __restrict__ bias,          // [8]
    float* __restrict__ y,                   // [D][H][W][8] fp32
    int D, int H, int W, int nb
    ) {
    using namespace c48t;
    __shared__ __attribute__((aligned(16))) unsigned short buf[2 * BUF_E];   // [half][piece][plane][hy][hx][8]
    __shared__ __attribute__((aligned(16))) float ex[NT_PLANES * NPOS * EXS];
    __shared__ int org[MAXT][4];   // origins of this block's tiles (three runtime divisions each: once, not per step)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool consumer = __builtin_amdgcn_readfirstlane(wave) < 4;   // wave-uniform by construction; tell the compiler
    const int nbx = (W + TX - 1) / TX, nby = (H + TY - 1) / TY;
    const int G = gridDim.x;
    const int ntile = (nb - (int)blockIdx.x + G - 1) / G;   // this block's tiles: blockIdx.x + j * G
    const size_t HW8 = (size_t)H * W * 8, V8 = (size_t)D * HW8;
    // tile index -> origin; every XCD owns a band of tile rows and walks it x-fastest, then row, then z
    // (conv0_w43_mfma); G is a multiple of 8 whenever nb is, so a block's tiles stay on its XCD's band
    auto origin = [&](int idx, int& x0, int& y0, int& z0) {
        int bx, by, bz;
        if (nby % 8 == 0 && G % 8 == 0) {
            const int xcd = idx & 7, rows = nby >> 3;
            int i = idx >> 3;
            bx = i % nbx; i /= nbx;
            by = xcd * rows + i % rows;
            bz = i / rows;
        } else {
            int b = idx;
            bx = b % nbx; b /= nbx;
            by = b % nby;
            bz = b / nby;
        }
        x0 = bx * TX; y0 = by * TY; z0 = bz * TZ;
    };

    for (int j = tid; j < ntile; j += 512) {
        int x0, y0, z0;
        origin((int)blockIdx.x + j * G, x0, y0, z0);
        org[j][0] = x0; org[j][1] = y0; org[j][2] = z0;
    }
    __syncthreads();
    const int ptid = tid & 255;

    // The two roles run DISJOINT loops (each with the same number of block barriers: one per half-step plus the one
    // after the prologue), so that the register allocator overlays the producers' staging registers with the
    // consumers' B fragments and accumulators instead of keeping both alive.  A loop iteration is one tile = eight
    // half-steps s = 2 c + h (chunk c, half h; s is a compile-time constant; buffer h holds planes 3 h .. 3 h + 2).
    // EVERY vector-memory instruction is unconditional -- the loads beyond a block's last step re-read its last tile,
    // the B fragments wrap around -- because one branch around a VMEM instruction makes hipcc wait for the loads it has
    // just issued (round 4: `if (s + 2 < S) issue_loads` -> s_waitcnt vmcnt(8) / (1) / (0) right after the new loads:
    // every step paid a full L2-miss latency).
    if (consumer) {
        // ---------------- consumer ----------------
        // units of a half-step: (plane 0..2 of the buffer, row pair 0..3); wave cw takes units 0, 1 = (pa, ra), (pa,
        // ra + 1) and unit 2 = (pb, rb): w0 (0,0) (0,1) (1,0), w1 (0,2) (0,3) (1,1), w2 (1,2) (1,3) (2,0), w3 (2,1)
        // (2,2) (2,3) -- every wave needs the B fragments of at most two planes and runs the same code.
        // Lane (r, g): halo x = 2 r + g.
        const int r = lane & 15, g = lane >> 4, cw = wave;
        const int pa = (0x2100 >> (4 * cw)) & 15, ra = (0x1220 >> (4 * cw)) & 15;
        const int pb = (0x2211 >> (4 * cw)) & 15, rb = (0x3010 >> (4 * cw)) & 15;
        const int upl[3] = {pa, pa, pb}, urp[3] = {ra, ra + 1, rb};
        int aoff[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) aoff[i] = upl[i] * PLANE_E + ((2 * urp[i]) * HX + 2 * r + g) * 8;
        // B fragments by raw buffer loads: the lane's 16 bytes + the plane in the vector offset, the fragment in the
        // scalar offset -- plain pointers made hipcc materialise (and spill) 35 64-bit addresses
        u32x4 B[2][2][3][3];   // two sets: the next step's 18 fragments are requested during a step
        const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<unsigned short*>(bp), (short)0, 4 * NT_PLANES * 9 * 1024, 0x00020000);
        const unsigned bvoff[2] = {(unsigned)lane * 16u + (unsigned)pa * 9u * 1024u,
                                   (unsigned)lane * 16u + (unsigned)pb * 9u * 1024u};
#pragma unroll
        for (int f = 0; f < 18; ++f)
            B[0][f / 9][(f / 3) % 3][f % 3] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(
                brs, (int)bvoff[f / 9], (int)(bstep(0) + (unsigned)(f % 9) * 1024u), 0));
        f32x4 acc[2][3][2];   // [half][unit][row of the pair]
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int n = 0; n < 2; ++n) acc[h][i][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
        // acc[h][i][rr][e] = (plane 3 h + upl[i], row 2 urp[i] + rr, x = 2 (4 g + e) + jj, channel co), n = lane & 15 = (jj, co)
        auto exchange = [&]() {
            const int n = lane & 15, jj = n >> 3, co = n & 7;
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int rr = 0; rr < 2; ++rr)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            ex[((3 * h + upl[i]) * NPOS + (2 * urp[i] + rr) * TX + 2 * (4 * g + e) + jj) * EXS + co] = acc[h][i][rr][e];
                            acc[h][i][rr][e] = 0.0f;
                        }
        };
        // output transform + stores of a finished tile, half `it` of it: thread -> (position, 4 channels).  Raw buffer
        // stores: `live` = false (a block's first tile has no predecessor) or a position outside the volume puts the
        // offset beyond the descriptor and the hardware drops the store -- no branch around a VMEM instruction
        const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(y, (short)0, (int)(V8 * 4), 0x00020000);
        const f32x4 obias = *reinterpret_cast<const f32x4*>(bias + (ptid & 1) * 4);
        auto output = [&](int j, int it, bool live) {   // j-th tile of this block
            const int x0 = org[j][0], y0 = org[j][1], z0 = org[j][2];
            const int pos = (ptid >> 1) + it * (NPOS / 2), ch = ptid & 1;
            const int gy = y0 + (pos >> 5), gx = x0 + (pos & 31);
            const bool ok = live && gy < H && gx < W;
            f32x4 M[NT_PLANES];
#pragma unroll
            for (int q = 0; q < NT_PLANES; ++q) M[q] = *reinterpret_cast<const f32x4*>(ex + (q * NPOS + pos) * EXS + ch * 4);
            const f32x4 s12 = M[1] + M[2], d12 = M[1] - M[2], s34 = M[3] + M[4], d34 = M[3] - M[4];
            f32x4 o[TZ];
            o[0] = (M[0] + s12) + s34;
            o[1] = d12 + 2.0f * d34;
            o[2] = s12 + 4.0f * s34;
            o[3] = (d12 + 8.0f * d34) + M[5];
            const unsigned base = (unsigned)((((size_t)z0 * H + gy) * W + gx) * 8 + ch * 4) * 4u;
#pragma unroll
            for (int q = 0; q < TZ; ++q) {
                const f32x4 v = relu(o[q] + obias);
                const unsigned off = (ok && z0 + q < D) ? base + (unsigned)q * (unsigned)(HW8 * 4) : 0xFFFFFFF0u;
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), yrs, (int)off, 0, 0);
            }
        };
        int kk = 0;
        auto cstep = [&](auto s_tag) {
            constexpr int s = decltype(s_tag)::value, h = s & 1;
            // the tile finished a step ago: output transform + stores in two halves (the consumers wait for the
            // producers at every barrier)
            if (s == 1 || s == 3) output(kk > 0 ? kk - 1 : 0, s >> 1, kk > 0);
            c48t_step_mfmas(buf + h * BUF_E, aoff, B[h], B[h ^ 1], brs, bvoff,
                            s < 7 ? bofs(chunk_of(kk, (s + 1) >> 1), (s + 1) & 1) : bofs(chunk_of(kk + 1, 0), 0), acc[h]);
            if (s == 7) exchange();   // read during the next tile's steps 1 and 3 (after a barrier)
        };
        __syncthreads();
#pragma unroll 1
        for (int k = 0; k < ntile; ++k) {
            kk = k;
            cstep(std::integral_constant<int, 0>{});
            __syncthreads();
            cstep(std::integral_constant<int, 1>{});
            __syncthreads();
            cstep(std::integral_constant<int, 2>{});
            __syncthreads();
            cstep(std::integral_constant<int, 3>{});
            __syncthreads();
            cstep(std::integral_constant<int, 4>{});
            __syncthreads();
            cstep(std::integral_constant<int, 5>{});
            __syncthreads();
            cstep(std::integral_constant<int, 6>{});
            __syncthreads();
            cstep(std::integral_constant<int, 7>{});
            __syncthreads();
        }
        output(ntile - 1, 0, true);
        output(ntile - 1, 1, true);
    } else {
        // ---------------- producer ----------------
        __builtin_amdgcn_s_setprio(2);   // the producers are the critical path: their VALU wins the issue arbitration
        unsigned boff[CPT][NT_PLANES];
        int loff[CPT];            // in 8-byte units inside one (piece, plane)
        int chy[CPT], chx[CPT], crel[CPT];   // the column's halo row / column and its float offset from the tile origin
#pragma unroll
        for (int i = 0; i < CPT; ++i) {
            // threads beyond the 680 columns shadow the last column (same loads, same values to the same LDS address):
            // no branch inside the staging code
            const int col = min(ptid + i * 256, NCOL - 1);
            loff[i] = col;    // (v * 2 + half) = col
            const int half = col & 1, v = col >> 1;
            chx[i] = v % HX - 1;
            chy[i] = v / HX - 1;
            crel[i] = (chy[i] * W + chx[i]) * 8 + half * 4;
        }
        // per tile: 32-bit arithmetic only (the launcher guarantees < 2^31 bytes per chunk plane)
        auto set_tile = [&](int j) {   // j-th tile of this block
            const int x0 = org[j][0], y0 = org[j][1], z0 = org[j][2];
            const int hw8 = (int)HW8, tbase = (y0 * W + x0) * 8;
#pragma unroll
            for (int i = 0; i < CPT; ++i) {
                const int gy = y0 + chy[i], gx = x0 + chx[i];
                const bool ok = (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
                const int cb = tbase + crel[i];
#pragma unroll
                for (int q = 0; q < NT_PLANES; ++q) {
                    const int gz = z0 - 1 + q;   // wave-uniform
                    boff[i][q] = (ok && (unsigned)gz < (unsigned)D) ? (unsigned)(gz * hw8 + cb) * 4u
                                                                      : 0x80000000u;   // beyond the descriptor: zeros
                }
            }
        };
        auto rsrc = [&](int c) {
            return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x + (size_t)c * V8), (short)0, (int)(V8 * 4), 0x00020000);
        };
        f32x4 stg[CPT][NT_PLANES];   // the staged chunk
        f32x4 hold[CPT][NPL];        // U3..U5 of the chunk transformed a step ago
        auto put = [&](unsigned short* dstbuf, int i, int t, const f32x4 u) {
            u32x2 p1, p2, p3;
            split3x(u, p1, p2, p3);
            u32x2* dst = reinterpret_cast<u32x2*>(dstbuf) + t * (PLANE_E / 4) + loff[i];
            dst[0] = p1;
            dst[PIECE_E / 4] = p2;
            dst[2 * (PIECE_E / 4)] = p3;
        };
        // half 0: transform the staged chunk, U0..U2 into buffer 0, U3..U5 held; a column's registers are refilled
        // with chunk `cn` as soon as it is transformed, two loads per plane segment (as one burst the loads took
        // 1.8-2.5 k cycles to enter the CU's vector-memory queue, with the whole transform waiting behind them)
        auto process0 = [&](int cn) {
            const __amdgpu_buffer_rsrc_t rs = rsrc(cn);
#pragma unroll
            for (int i = 0; i < CPT; ++i) {
                f32x4 d[NT_PLANES];
#pragma unroll
                for (int q = 0; q < NT_PLANES; ++q) d[q] = stg[i][q];
                const f32x4 t1 = d[4] - 4.0f * d[2], t2 = d[3] - 4.0f * d[1];
                const f32x4 t3 = d[4] - d[2], t4 = 2.0f * (d[3] - d[1]);
                const f32x4 u0 = 4.0f * d[0] - 5.0f * d[2] + d[4];
                const f32x4 u1 = t1 + t2, u2 = t1 - t2;
                hold[i][0] = t3 + t4;
                hold[i][1] = t3 - t4;
                hold[i][2] = 4.0f * d[1] - 5.0f * d[3] + d[5];
                const f32x4 u[NPL] = {u0, u1, u2};
#pragma unroll
                for (int t = 0; t < NPL; ++t) {
#pragma unroll
                    for (int q = 2 * t; q < 2 * t + 2; ++q)
                        stg[i][q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)boff[i][q], 0, 0));
                    put(buf, i, t, u[t]);
                    // one plane at a time, in this order
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        };
        // half 1: the held U3..U5 into buffer 1
        auto process1 = [&]() {
#pragma unroll
            for (int i = 0; i < CPT; ++i)
#pragma unroll
                for (int t = 0; t < NPL; ++t) {
                    put(buf + BUF_E, i, t, hold[i][t]);
                    __builtin_amdgcn_sched_barrier(0);
                }
        };
        // half-step (k, s): h = 0 -> buffer 1 gets U3..U5 of step c's chunk; h = 1 -> buffer 0 gets U0..U2 of step c + 1's
        // chunk and step c + 2's chunk is loaded (chunk_of: the tile's chunk order) (chunks of the next tile from c = 2 on; after the last tile: re-reads of it, into a
        // buffer nobody reads)
        auto pstep = [&](int k, auto s_tag) {
            constexpr int s = decltype(s_tag)::value, c = s >> 1, h = s & 1;
            if (s == 5 && k + 1 < ntile) set_tile(k + 1);   // the loads below start the next tile
            if (h == 0) process1();
            else process0(c < 2 ? chunk_of(k, c + 2) : chunk_of(k + 1, c - 2));
        };
        // prologue: chunk 0 transformed (buffer 0 + held), chunk 1 in flight
        set_tile(0);
        {
            const __amdgpu_buffer_rsrc_t rs = rsrc(0);
#pragma unroll
            for (int i = 0; i < CPT; ++i)
#pragma unroll
                for (int q = 0; q < NT_PLANES; ++q)
                    stg[i][q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)boff[i][q], 0, 0));
        }
        process0(1);
        __syncthreads();
#pragma unroll 1
        for (int k = 0; k < ntile; ++k) {
            pstep(k, std::integral_constant<int, 0>{});
            __syncthreads();
            pstep(k, std::integral_constant<int, 1>{});
            __syncthreads();
            pstep(k, std::integral_constant<int, 2>{});
            __syncthreads();
            pstep(k, std::integral_constant<int, 3>{});
            __syncthreads();
            pstep(k, std::integral_constant<int, 4>{});
            __syncthreads();
            pstep(k, std::integral_constant<int, 5>{});
            __syncthreads();
            pstep(k, std::integral_constant<int, 6>{});
            __syncthreads();
            pstep(k, std::integral_constant<int, 7>{});
            __syncthreads();
        }
    }
}

int launch_conv0_wino43_split(const void* x, void* y, const void* bp, const float* bias, int D, int H, int W,
                              int dtype, hipStream_t s) {
    using namespace c48t;
    if (dtype != MVS_F32) return fail(MVS_ERR_BAD_DTYPE, "conv0_wino43_split: fp32 volumes only (dtype %d)", dtype);
    if ((size_t)D * H * W * 8 * 4 >= ((size_t)1 << 31))
        return fail(MVS_ERR_BAD_SHAPE, "conv0_wino43_split: plane of %zu bytes exceeds 31-bit buffer offsets",
                    (size_t)D * H * W * 8 * 4);
    const int nb = ((W + TX - 1) / TX) * ((H + TY - 1) / TY) * ((D + TZ - 1) / TZ);
    const int cus = device_cus();
    int grid = nb < cus ? nb : cus;
    if ((nb + grid - 1) / grid > MAXT) grid = (nb + MAXT - 1) / MAXT;   // (> 130 k tiles: never at 31-bit volumes)
    conv0_w48t_kernel<<<grid, 512, 0, s>>>(static_cast<const float*>(x), static_cast<const unsigned short*>(bp), bias,
                                           static_cast<float*>(y), D, H, W, nb);
    return check_hip(hipGetLastError(), "conv0_w48t launch");
}

// ---------------------------------------------------------------------------------------------
// host: wfold [27][32][8] (tap = kz*9 + ky*3 + kx) -> bp [4 chunks][6 t][3 ky][3 pieces][64 lanes][8] bf16.
// The z taps are transformed by G of F(4,3) in double and rounded once to fp32 (the values conv0_w43_mfma uses),
// then split into three bf16 pieces.  Lane (n = lane & 15, g = lane >> 4), element j: k = (halo x offset g,
// channel j of the chunk), column n = (x-output jj = n >> 3 of the pair, co = n & 7); tap kx = g - jj.
// ---------------------------------------------------------------------------------------------
static inline uint16_t bf16_rne(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    if ((u & 0x7F800000u) == 0x7F800000u && (u & 0x007FFFFFu)) return (uint16_t)((u >> 16) | 0x0040u);  // NaN
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
static inline float bf16_to_f32(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
    float v;
    std::memcpy(&v, &u, 4);
    return v;
}

void pack_conv0_wino43_split_weights(const float* wfold, void* out) {
    uint16_t* bp = static_cast<uint16_t*>(out);
    for (int c = 0; c < 4; ++c)
        for (int t = 0; t < 6; ++t)
            for (int ky = 0; ky < 3; ++ky)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int n = lane & 15, g = lane >> 4, jj = n >> 3, co = n & 7, kx = g - jj;
                        float gv = 0.0f;
                        if (kx >= 0 && kx <= 2) {
                            const int tap = ky * 3 + kx, ci = 8 * c + j;
                            const double g0 = wfold[((size_t)(0 * 9 + tap) * 32 + ci) * 8 + co];
                            const double g1 = wfold[((size_t)(1 * 9 + tap) * 32 + ci) * 8 + co];
                            const double g2 = wfold[((size_t)(2 * 9 + tap) * 32 + ci) * 8 + co];
                            double gd;
                            switch (t) {
                                case 0: gd = g0 / 4.0; break;
                                case 1: gd = -(g0 + g1 + g2) / 6.0; break;
                                case 2: gd = -(g0 - g1 + g2) / 6.0; break;
                                case 3: gd = g0 / 24.0 + g1 / 12.0 + g2 / 6.0; break;
                                case 4: gd = g0 / 24.0 - g1 / 12.0 + g2 / 6.0; break;
                                default: gd = g2; break;
                            }
                            gv = (float)gd;
                        }
                        const uint16_t h1 = bf16_rne(gv);
                        const float r1 = gv - bf16_to_f32(h1);
                        const uint16_t h2 = bf16_rne(r1);
                        const float r2 = r1 - bf16_to_f32(h2);
                        const uint16_t h3 = bf16_rne(r2);
                        const uint16_t hs[3] = {h1, h2, h3};
                        for (int q = 0; q < 3; ++q)
                            bp[((((size_t)(c * 6 + t) * 3 + ky) * 3 + q) * 64 + lane) * 8 + j] = hs[q];
                    }
}

}  // namespace mvs
