// launch_plan.h -- where every launch of the depth path is planned: which kernel form runs a CostRegNet layer, the
// fused tail and the warp, with which block tile, and how the z-marching launchers and the tap-cache warp cut the
// volume.  Pure host functions of the shape, the storage type, the switches and the CU count: plain C++17, no HIP
// header, no environment read, no HIP call (tests/plan_sweep.cpp compiles this file alone with a host compiler).
// The launchers (the .hip files) ask the planner and switch over its answer; a refusal stays with its launcher.
// DESIGN.md, "Where a launch is planned", says how a test asks (mvs_test_launch_plan at the end of this file).
#pragma once
#include <cstddef>
#include <initializer_list>

#include "mvs_abi.h"

namespace mvs {

// CostRegNet layer table (models/mvsnet.py:35-62).
enum LayerKind { kConv = 0, kDeconv = 1 };
struct LayerSpec {
    int cin, cout, stride, kind;
    int level_in, level_out;  // resolution level: voxel dims = (D,h,w) >> level
};
constexpr LayerSpec kLayers[MVS_NUM_LAYERS] = {
    {32, 8, 1, kConv, 0, 0},     // 0 conv0
    {8, 16, 2, kConv, 0, 1},     // 1 conv1
    {16, 16, 1, kConv, 1, 1},    // 2 conv2
    {16, 32, 2, kConv, 1, 2},    // 3 conv3
    {32, 32, 1, kConv, 2, 2},    // 4 conv4
    {32, 64, 2, kConv, 2, 3},    // 5 conv5
    {64, 64, 1, kConv, 3, 3},    // 6 conv6
    {64, 32, 2, kDeconv, 3, 2},  // 7 conv7  (+conv4)
    {32, 16, 2, kDeconv, 2, 1},  // 8 conv9  (+conv2)
    {16, 8, 2, kDeconv, 1, 0},   // 9 conv11 (+conv0)
    {8, 1, 1, kConv, 0, 0},      // 10 prob (bias, no BN / ReLU)
};

// Kernel-selection switches (environment variables MVS_*), read once on first use by options() (mvs_host.hip; DESIGN.md
// lists why each exists).  Unless noted, a bool switch is on by default and "0" (first character) turns it off.
struct Options {
    bool conv0_wino;              // MVS_CONV0_WINO: conv0 as Winograd F(4,3) along z; off = the direct 4x4x1 MFMA form
    bool conv_wino;               // MVS_CONV_WINO: conv2 / conv4 as Winograd F(2,3) along z (fp32 MFMA path)
    bool conv0_split;             // MVS_CONV0_SPLIT: conv0 of fp32 volumes with split bf16 operands; off = fp32 MFMA
    bool split_layers;            // MVS_SPLIT_LAYERS: conv2 .. conv4 (+ MVS_SPLIT_DECONV) of fp32 volumes, split operands
    bool mfma16;                  // MVS_MFMA16: 16-bit storage on the 16-bit matrix cores; off = fp32 MFMA arithmetic
    bool fuse_prob;               // MVS_FUSE_PROB: conv11 + prob as one kernel; off = two launches
    bool tail_split;              // MVS_TAIL_SPLIT: the fused tail of fp32 volumes with split operands; off = fp32 MFMA
    bool warp_tc;                 // MVS_WARP_TC: the tap-cache warp + variance kernel (fp32 features); off = plain gather
    bool warp_tc16;               // MVS_WARP_TC16: the same for 16-bit features
    bool force_direct;            // MVS_FORCE_DIRECT, "1" = on (default off): VALU direct kernels for every layer
    bool feat16;                  // MVS_FEAT16, "1" = on (default off): the 16-bit modes gather from a narrowed feature copy
    bool feat_split01;            // MVS_FEAT_SPLIT01, "1" = on (default off): FeatureNet conv0 and conv1 as two kernels
    int conv1z;                   // MVS_CONV1Z: fp32 conv1 z-marching kernel never (0) / always (1); -1 (unset) = by size
    int convz16;                  // MVS_CONVZ16: the same for the 16-bit conv1 .. conv3
    int conv0z16;                 // MVS_CONV0Z16: the same for the 16-bit conv0
    int deep_tiles;               // MVS_DEEP_TILES: z-deep 16-bit block tiles never (0) / always (1); -1 (unset) = by size
    int split_deconv;             // MVS_SPLIT_DECONV: split-operand transposed layers, bit 0 = conv7, bit 1 = conv9; default 2
    int persist_cus;              // MVS_PERSIST_CUS: > 0 replaces the CU count in conv3d_mfma.hip's persistent grid sizing
    // MVS_WARP_DEPTH_FASTEST, parsed two ways: the plain kernel forces the depth-slab-fastest order on "1" (default by
    // size); the tap-cache kernel takes its integer value, 1 / 0 = always / never, -1 (unset) = by size
    bool warp_depth_fastest;
    int warp_depth_fastest_tc;
};
constexpr int kNumOptions = 20;
constexpr Options default_options() {
    return Options{true, true, true, true, true, true, true, true, true, false, false, false, -1, -1, -1, -1, 2, 0, false, -1};
}

// Upper ends of the shape domain (include/mvs_abi.h states them per entry point), from the kernels' index types:
//  - the per-pixel ops (soft-argmin, depth regression, the soft-argmin backward) hold h*w and the pixel index of the
//    last, partly filled block in an int: h*w + 255 (the largest block of the three) must not wrap
//  - the soft-argmin's depth index travels as a float (sum_d p_d * d, then trunc): exact up to 2^24
//  - every CostRegNet kernel form addresses one 8-channel plane of its INPUT with int offsets ("plane exceeds 31-bit
//    offsets" in the MFMA launchers); planes are told apart and outputs addressed with size_t
constexpr size_t kMaxPixels = ((size_t)1 << 31) - 256;
constexpr int kMaxSoftargminD = 1 << 24;
constexpr size_t kMaxConvInputVoxels = ((size_t)1 << 28) - 1;   // Di*Hi*Wi*8 < 2^31
//  - prob_lds (layer 10) keeps a piece's offset from its tile's halo origin in an int: up to 5 planes, 9 rows and 33
//    voxels on, whatever D and H are: ((5 Hi + 9) Wi + 33) * 8 + 4 < 2^31
constexpr size_t kMaxProbHaloVoxels = ((size_t)1 << 28) - 1;
//  - mvs_homo_warp: one thread per (d, y, x), 256 to a block, fewer than 2^31 blocks; element offsets are size_t
constexpr size_t kMaxHomoWarpThreads = (((size_t)1 << 31) - 2) * 256;
constexpr size_t kMaxHomoWarpOutput = (size_t)1 << 61;

namespace plan {

// ---- tile constants the geometry depends on: the kernels take them from here ----
constexpr int kC1zTYO = 8, kC1zTXO = 16;     // conv1z (conv3d_mfma.hip): output column of a block, 4 x 2 M-tiles of 2 x 8
constexpr int kConvZ16TY = 8;                // convz16 (conv3d_mfma16.hip): output column TY x TX
constexpr int convz16_tx(int S) { return S == 1 ? 32 : 16; }
// C0Z_TY = rows (= waves) per block of conv0z16: 8 -> one block per CU (default); 4 -> two independent 4-wave blocks per CU
// (-DC0Z_TY=4) measured slower: 0.632 vs 0.590 ms at cfg3, 0.0876 vs 0.0818 at cfg5 (halo 1.5x instead of 1.25x in y)
#ifndef C0Z_TY
#define C0Z_TY 8
#endif
constexpr int kC0zTY = C0Z_TY, kC0zTX = 32;
constexpr int kCpBY = 4, kCpBX = 2;          // conv11_prob: MFMA M-tiles (2 rows x 8 columns of input voxels) per block
constexpr int kCpPY = 4 * kCpBY - 2, kCpPX = 16 * kCpBX - 2;   // logits per tile: 14 x 30
// tap-cache warp (warp_variance_tc.hip): slab candidates in order of preference, all multiples of 4 and <= kMaxSlab
constexpr int kTcSlabs[] = {40, 44, 36, 32, 28, 24};
constexpr int kMaxSlab = 44;
constexpr int kTcPix = 32;                   // pixels per block: 256 threads / 8 lanes per pixel (4 channels per thread)
// the fp32 persistent tile kernel of conv1 (ConvG<8, 16, 2, 1, 2, 2>): floats of its LDS tile
constexpr int kConv1TileFloats = 3 * 9 * 40 * 12;

constexpr long cdiv(long a, long b) { return (a + b - 1) / b; }
constexpr int out_dim(int i, int stride) { return (i - 1) / stride + 1; }

// ---- the one z split ----
struct ZSplit {
    int zc;      // planes per chunk (depths per slab)
    int n;       // chunks
    int last;    // planes of the last chunk
    long grid;   // blocks launched: columns x chunks
};
inline ZSplit z_split(int dz, int zc, long cols) {
    const int n = (int)cdiv(dz, zc);
    return ZSplit{zc, n, dz - (n - 1) * zc, cols * n};
}
// The chunk count nz in 1..nz_max with the best fill of the last round of `slots` resident blocks, discounted by a
// per-chunk prologue of `prologue` steps; the first best wins.  Returns the chunk size ceil(dz / nz).
inline int best_z_chunk(int dz, long blocks_per_chunk, long slots, int nz_max, double prologue) {
    int best = 1;
    double best_fill = 0.0;
    for (int nz = 1; nz <= nz_max; ++nz) {
        const int zc = (int)cdiv(dz, nz), nzc = (int)cdiv(dz, zc);
        const long nb = blocks_per_chunk * nzc;
        const double fill = (double)nb / (double)(cdiv(nb, slots) * slots) * zc / (zc + prologue);
        if (fill > best_fill + 1e-9) { best_fill = fill; best = nz; }
    }
    return (int)cdiv(dz, best);
}
inline ZSplit best_z_split(int dz, long blocks_per_chunk, long slots, int nz_max, double prologue) {
    return z_split(dz, best_z_chunk(dz, blocks_per_chunk, slots, nz_max, prologue), blocks_per_chunk);
}

// ---- kernel forms ----
enum Form {
    kNone = 0,          // no kernel covers the layer: the launcher refuses
    kDirect,            // VALU direct kernels, every layer (conv3d_direct.hip; MVS_FORCE_DIRECT=1)
    kProbLds,           // prob (layer 10), every storage type (conv3d_direct.hip)
    kConv0WinoSplit,    // conv0, Winograd F(4,3) along z, split bf16 operands (conv0_split.hip)
    kConv0Wino,         // conv0, Winograd F(4,3) along z on the 4x4x1 MFMA (conv_winograd.hip)
    kConv0Mfma,         // conv0, direct 4x4x1 MFMA form (conv3d_mfma.hip)
    kConv0Tile16,       // conv0, 16-bit tile kernel (conv3d_mfma16.hip)
    kConv0Z16,          // conv0, 16-bit z-marching kernel
    kConv1Z,            // conv1, fp32 z-marching kernel (conv3d_mfma.hip)
    kConvGPersist,      // conv1, fp32 MFMA tile kernel as persistent blocks
    kConvG,             // conv1 .. conv4, fp32 MFMA tile kernel, one tile per block
    kConvWz,            // conv2 / conv4, Winograd F(2,3) along z (conv_winograd.hip)
    kConvS,             // conv5 / conv6, all-K-resident split-K (conv3d_small.hip)
    kDeconvS,           // conv7, the same
    kDeconvG,           // conv9 / conv11, fp32 MFMA transposed tile kernel (conv3d_mfma.hip)
    kConvZ16,           // conv1 .. conv3, 16-bit z-marching kernel (conv3d_mfma16.hip)
    kConvG16,           // conv1 .. conv6, 16-bit tile kernel
    kDeconvG16,         // conv7 / conv9 / conv11, 16-bit transposed tile kernel
    kConvGSplit,        // conv2 .. conv4 of fp32 volumes, split operands on the 16-bit tile kernel
    kDeconvGSplit,      // conv7 / conv9 of fp32 volumes, the same
    kTailTwoLaunches,   // conv11 and prob as layers 9 and 10
    kTailSplit,         // fused tail, fp32 volumes, split operands (conv11_prob.hip)
    kTailPriv,          // fused tail, fp32 volumes, fp32 MFMA
    kTail16,            // fused tail, 16-bit volumes
    kWarpTc,            // tap-cache warp + variance (warp_variance_tc.hip), fp32 or 16-bit feature copy
    kWarpPlain,         // plain gather warp + variance (warp_variance.hip), fp32 or 16-bit feature copy
};

struct Plan {
    Form form = kNone;
    int bz = 0, by = 0, bx = 0;    // block tile of the 16-bit tile kernels, in M-tiles of 2 x 8 voxels
    ZSplit z{0, 0, 0, 0};          // z-marching forms and the tap-cache warp; grid == 0: the launcher sizes its own grid
    int nbx = 0, nby = 0;          // columns of the z-marching forms; the tap-cache warp: pixel blocks in nbx
    int depth_fastest = 0;         // warps: depth slabs vary fastest in the block order
};
inline Plan tiled(Form f, int bz, int by, int bx) {
    Plan p;
    p.form = f; p.bz = bz; p.by = by; p.bx = bx;
    return p;
}
inline Plan formed(Form f) { return tiled(f, 0, 0, 0); }
inline Plan marched(Form f, int nbx, int nby, const ZSplit& z) {
    Plan p = formed(f);
    p.nbx = nbx; p.nby = nby; p.z = z;
    return p;
}

constexpr size_t k2_31 = (size_t)1 << 31, k2_32 = (size_t)1 << 32;

// Does a grid of bz x by x bx M-tiles (2 x 8 outputs each) over the OUTPUT of a stride-S layer (S = 1 with the input dims
// for the transposed layers) still give every CU a block and a half?  MVS_DEEP_TILES=1 / 0: always / never.
inline bool tile_fills_chip(int Di, int Hi, int Wi, int S, int bz, int by, int bx, const Options& opt, int cus) {
    if (opt.deep_tiles >= 0) return opt.deep_tiles != 0;
    const long nb = cdiv(out_dim(Wi, S), 8 * bx) * cdiv(out_dim(Hi, S), 2 * by) * cdiv(out_dim(Di, S), bz);
    return 2 * nb >= 3 * (long)cus;
}

// Block tiles of the tile kernels of conv3d_mfma16.hip per layer, in M-tiles of 2 x 8 voxels.  16-bit storage: [0] the
// default and [1] the z-deep tile that runs where tile_fills_chip says so (the same where there is no choice).
// cfg5 sweep of conv3: 1x2x2 0.0115, 4x1x1 0.0107 ms.
// conv4 .. conv6: z-deep block tiles (halo planes re-used) wherever they still give every CU a block and a half --
// round-4 sweep, cfg3 bf16 (1600x1184x256): conv4 1x2x2 -> 4x2x1 0.0574 -> 0.0456 ms, conv5 1x1x1 -> 2x1x1 0.0296 -> 0.0236,
// conv6 1x1x1 -> 4x1x1 0.0479 -> 0.0243; cfg5 fp16 (640x512x192): conv4 0.0133 -> 0.0118, conv5 / conv6 keep 1x1x1
// (2x1x1 / 4x1x1 would leave 240 / 120 blocks for 256 CUs: 0.0104 / 0.0145 against 0.0106 / 0.0134).
// The same for the transposed layers (tiles over the INPUT grid): cfg3 conv7 1x1x1 -> 2x1x1 0.0486 -> 0.0389, conv9 1x4x1
// -> 4x2x1 0.1059 -> 0.1026; cfg5 conv9 0.0171 -> 0.0164, conv7 stays (2x1x1: 240 blocks).
struct Tile { int bz, by, bx; };
constexpr Tile kTiles16[10][2] = {
    {{0, 0, 0}, {0, 0, 0}},   // conv0: its own kernels
    {{2, 2, 2}, {2, 2, 2}}, {{2, 4, 2}, {2, 4, 2}}, {{4, 1, 1}, {4, 1, 1}},   // conv1 .. conv3
    {{1, 2, 2}, {4, 2, 1}}, {{1, 1, 1}, {2, 1, 1}}, {{1, 1, 1}, {4, 1, 1}},   // conv4 .. conv6
    {{1, 1, 1}, {2, 1, 1}}, {{1, 4, 1}, {4, 2, 1}}, {{1, 4, 2}, {1, 4, 2}},   // conv7, conv9, conv11
};
// fp32 volumes, split operands (which layers, and the sweeps behind these tiles: plan_layer)
constexpr Tile kTilesSplit[10] = {{0, 0, 0}, {0, 0, 0}, {2, 4, 2}, {2, 2, 1}, {4, 2, 1}, {0, 0, 0}, {0, 0, 0}, {1, 1, 1}, {2, 4, 1}, {0, 0, 0}};
// Is bz x by x bx a tile the planner reports for the layer with these channels?  run_convg16 / run_deconvg16 assert it of
// every instantiation, so a tile edited in a launcher and not here (or here and not there) does not build.
constexpr bool tile_is_planned(int cin, int cout, int kind, int bz, int by, int bx) {
    for (int l = 1; l < 10; ++l) {
        if (kLayers[l].cin != cin || kLayers[l].cout != cout || kLayers[l].kind != kind) continue;
        for (const Tile& t : {kTiles16[l][0], kTiles16[l][1], kTilesSplit[l]})
            if (t.bz == bz && t.by == by && t.bx == bx) return true;
    }
    return false;
}

// Layers 0 .. 9 of a 16-bit volume on the 16-bit matrix cores (conv3d_mfma16.hip).
inline Plan plan_layer16(int layer, int Di, int Hi, int Wi, const Options& opt, int cus) {
    const size_t vox = (size_t)Di * Hi * Wi;
    if (layer == 0) {
        // z-marching kernel once its (y, x) columns can fill the chip; MVS_CONV0Z16=0 keeps the tile kernel (A/B runs),
        // 1 = also at small shapes (tests)
        const int nbx = (int)cdiv(Wi, kC0zTX), nby = (int)cdiv(Hi, kC0zTY);
        const long ncol = (long)nbx * nby;
        if (opt.conv0z16 != 0 && Di >= 8 && vox * 16 < k2_32 - 64 &&
            (opt.conv0z16 == 1 || (size_t)ncol * (Di / 8) >= (size_t)cus / 2))
            // z chunks (>= 8 planes each; every chunk re-reads 2 planes): the split that fills the last round of the
            // blocks resident at once best
            return marched(kConv0Z16, nbx, nby, best_z_split(Di, ncol, (long)cus * (8 / kC0zTY), Di / 8, 2.0));
        return formed(kConv0Tile16);
    }
    if (layer >= 1 && layer <= 3 && opt.convz16 != 0) {
        // layers 1..3 through the z-marching kernel when their columns fill the chip (MVS_CONVZ16=0/1 = never / always)
        const int S = kLayers[layer].stride, cout = kLayers[layer].cout;
        const int Do = out_dim(Di, S), Ho = out_dim(Hi, S), Wo = out_dim(Wi, S);
        const int nbx = (int)cdiv(Wo, convz16_tx(S)), nby = (int)cdiv(Ho, kConvZ16TY);
        const long ncol = (long)nbx * nby;
        bool take = !((size_t)Do * Ho * Wo * cout * 2 >= k2_32 - 64 || Do < 4);
        // enough columns x 8-plane chunks to fill the chip (cfg5's conv3 -- 12 columns of 48 planes -- measured 0.016 vs
        // 0.012 ms for the tile kernel: short chunks pay the two-step prologue too often)
        if (opt.convz16 != 1 && ncol * (Do / 8) * 4 < (long)cus * 3) take = false;
        // round 4, after the tile kernels got z-deep tiles, the XCD-aware order and staged epilogues: conv3 is faster on the tile
        // kernel at every bench size (cfg3 0.0433-0.0448 against 0.0456-0.0463 ms, cfg5 0.0108 against 0.0154), conv2 on it at cfg5's
        // size (0.0178 against 0.0204-0.0214) but not at cfg3's (0.106 against 0.087); conv1 stays here (cfg5 0.0215 / 0.0256, cfg3
        // 0.113 / 0.148)
        if (opt.convz16 != 1 && (layer == 3 || (layer == 2 && ncol * (Do / 8) < (long)cus * 3))) take = false;
        // z chunks of >= 4 output planes: best fill of the last round of one block per CU
        if (take) return marched(kConvZ16, nbx, nby, best_z_split(Do, ncol, cus, (Do + 3) / 4, 2.5));
    }
    if (layer < 1 || layer > 9) return formed(kNone);
    const Tile& d = kTiles16[layer][1];
    const bool deep = tile_fills_chip(Di, Hi, Wi, kLayers[layer].kind == kConv ? kLayers[layer].stride : 1, d.bz, d.by, d.bx, opt, cus);
    const Tile& t = kTiles16[layer][deep ? 1 : 0];
    return tiled(layer <= 6 ? kConvG16 : kDeconvG16, t.bz, t.by, t.bx);
}

// fp32 conv1, and conv1 of a 16-bit volume under MVS_MFMA16=0 (conv3d_mfma.hip).  `cus` here is MVS_PERSIST_CUS where set.
inline Plan plan_conv1(int Di, int Hi, int Wi, int dtype, const Options& opt, int cus) {
    const int pcus = opt.persist_cus > 0 ? opt.persist_cus : cus;
    const int Do = out_dim(Di, 2), Ho = out_dim(Hi, 2), Wo = out_dim(Wi, 2);
    const size_t vox = (size_t)Di * Hi * Wi;
    // fp32 storage, a volume whose (y, x) columns fill the chip: the z-marching kernel (MVS_CONV1Z=0/1 = never / always);
    // else the persistent tile kernel
    const int nbx = (int)cdiv(Wo, kC1zTXO), nby = (int)cdiv(Ho, kC1zTYO);
    const long ncol = (long)nbx * nby;
    if (dtype == MVS_F32 && opt.conv1z != 0 && (size_t)Do * Ho * Wo * 16 * 4 < k2_32 - 64 && vox * 8 < k2_31 &&
        (opt.conv1z == 1 || ncol * ((Do + 3) / 4) >= pcus / 2))
        // z chunks (>= 4 output planes; each chunk re-reads one input plane and pays a prologue of about two steps): the
        // split that fills the last round of one-block-per-CU best
        return marched(kConv1Z, nbx, nby, best_z_split(Do, ncol, pcus, (Do + 3) / 4, 2.5));
    // persistent blocks: as many per CU as the LDS tile allows (at most 4) -- only when every block gets several tiles;
    // otherwise the one-tile-per-block kernel balances better and is leaner (conv3: 1,152 tiles measured 0.037 vs 0.032 ms)
    const long ntiles = cdiv(Wo, 16) * cdiv(Ho, 4) * Do;   // 1 x 2 x 2 M-tiles
    int per_cu = (int)((160 * 1024) / (sizeof(float) * kConv1TileFloats + 512));
    per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);
    const long nblocks = (long)pcus * per_cu;
    Plan p = formed(ntiles < 4 * nblocks ? kConvG : kConvGPersist);
    p.z.grid = p.form == kConvGPersist ? nblocks : 0;
    return p;
}

// Which kernel form runs CostRegNet layer `layer` on an input of Di x Hi x Wi voxels, and with which tile / z split.
inline Plan plan_layer(int layer, int Di, int Hi, int Wi, int dtype, const Options& opt, int cus) {
    if (layer < 0 || layer >= MVS_NUM_LAYERS) return formed(kNone);
    // MVS_FORCE_DIRECT=1 routes every layer through the direct kernels (A/B checks in tests)
    if (opt.force_direct) return formed(kDirect);
    // 16-bit storage: 16-bit MFMA arithmetic (conv3d_mfma16.hip) unless MVS_MFMA16=0 asks for fp32 arithmetic on the
    // narrowed operands
    if (opt.mfma16 && (dtype == MVS_F16 || dtype == MVS_BF16) && layer <= 9) return plan_layer16(layer, Di, Hi, Wi, opt, cus);
    if (layer == 0) {
        // conv0: Winograd F(4,3) along z on the 4x4x1 MFMA (1/2 of the direct form's MFMAs; conv_winograd.hip)
        // unless MVS_CONV0_WINO=0 asks for the direct form (cross-check) or the volume needs 64-bit offsets
        // fp32 volumes: the same F(4,3) scheme with every operand split into three bf16 pieces, six cross products per
        // fp32 product on the bf16 matrix cores, fp32 accumulation (conv0_split.hip: fp32-equivalent arithmetic -- the
        // per-layer bounds of the fp32 kernel hold unchanged -- at 0.28 instead of 0.36 ms).  MVS_CONV0_SPLIT=0: the
        // fp32-MFMA Winograd kernel
        if (opt.conv0_wino && Di % 4 == 0 && (size_t)Di * Hi * Wi * 32 < k2_31)
            return formed(opt.conv0_split && dtype == MVS_F32 ? kConv0WinoSplit : kConv0Wino);
        return formed(kConv0Mfma);
    }
    // fp32 volumes: the level-1 .. 3 layers on the bf16 matrix cores with split operands (conv3d_mfma16.hip, round 4) unless
    // MVS_SPLIT_LAYERS=0 keeps the fp32-MFMA kernels below: conv2, conv3, conv4 (measured at cfg2 against the fp32-MFMA
    // kernels: 0.0588 -> 0.0534, 0.0310 -> 0.0276, 0.0396 -> 0.0329 ms with the 16-bit kernels' block tiles; a sweep of 8-20
    // tiles per layer (tools/gpu/tile_sweep.sh, BZ x BY x BX M-tiles of 2 x 8 outputs): conv3 1x2x2 -> 2x2x1 0.0275 -> 0.0238,
    // conv4 1x2x2 -> 4x2x1 0.0325 -> 0.0254 -- z-deep, x-narrow tiles re-use the halo planes --, conv2 stays at 2x4x2).
    // Measured and NOT selected: conv5 / conv6 on this tile kernel (0.0182 / 0.0289 against 0.0176 / 0.0242 ms for the
    // all-K-resident split-K fp32 kernels: on 7,680 voxels the chunk pipeline is the cost, not the matrix pipe), conv1 on it
    // (0.083 ms) and as a z-marching kernel with three bf16 rings (csrc/attic/conv1_split_zmarch.hip in commit c2f08ac: 0.054
    // against 0.046 ms for the fp32-MFMA z-marching kernel).
    // conv9 likewise (deconvgs<32, 16, 2, 4, 1>: 0.0354 -> 0.0266 ms at cfg2; tiles of 1x4x1 / 2x2x1 / 1x2x2 / 1x2x1 M-tiles per
    // block: 0.0278 / 0.0277 / 0.0301 / 0.0316); conv7 on the same kernel measured 0.0248 against 0.0234 ms for the split-K
    // fp32 kernel and is not selected (MVS_SPLIT_DECONV: bit 0 = conv7, bit 1 = conv9; default 2).
    if (opt.split_layers && dtype == MVS_F32) {
        const bool covered = (layer >= 2 && layer <= 4) || (layer == 7 && (opt.split_deconv & 1)) || (layer == 8 && (opt.split_deconv & 2));
        if (covered) return tiled(layer <= 4 ? kConvGSplit : kDeconvGSplit, kTilesSplit[layer].bz, kTilesSplit[layer].by, kTilesSplit[layer].bx);
    }
    // stride-1 layers conv2 / conv4: Winograd F(2,3) along z (conv_winograd.hip) unless MVS_CONV_WINO=0.  conv6 (64 -> 64
    // on 7,680 voxels) stays direct: with two-plane tiles it has only 240 blocks for 256 CUs and measured 0.035 vs 0.033 ms.
    if ((layer == 2 || layer == 4) && opt.conv_wino) return formed(kConvWz);
    // the 1/8-resolution layers conv5 / conv6 / conv7: all-K-resident split-K kernels (conv3d_small.hip).  The
    // 1/4-resolution layers measured SLOWER in this scheme at cfg2 (3,840 M-tiles = 3.75 rounds of blocks; conv3 0.034 vs
    // 0.031 ms, conv4 direct 0.045 vs 0.039 Winograd, conv9 0.041 vs 0.035): with several rounds per CU the chunk pipeline
    // of co-resident blocks overlaps well enough, and the wider blocks only lose occupancy.
    if (layer == 5 || layer == 6) return formed(kConvS);
    if (layer == 7) return formed(kDeconvS);
    if (layer == 1) return plan_conv1(Di, Hi, Wi, dtype, opt, cus);
    if (layer <= 4) return formed(kConvG);
    if (layer <= 9) return formed(kDeconvG);
    return formed(kProbLds);
}

// The fused tail's kernel form and z split on d9 = Di x Hi x Wi (conv11_prob.hip); chunks count INPUT planes.
inline Plan plan_conv11_prob(int Di, int Hi, int Wi, int dtype, const Options& opt, int cus) {
    const long nbx = cdiv(2 * (long)Wi - 2, kCpPX) > 0 ? cdiv(2 * (long)Wi - 2, kCpPX) : 1;
    const long nby = cdiv(2 * (long)Hi - 2, kCpPY) > 0 ? cdiv(2 * (long)Hi - 2, kCpPY) : 1;
    // z chunks of >= 4 input planes (every chunk recomputes one input plane and pays a prologue of about half a step):
    // the split that fills the last round of two-blocks-per-CU best.  (Round 2 took the largest split that keeps all
    // blocks resident at once: fine at cfg2 (60 tiles x 8 chunks = 480 blocks for 512 slots), 57 % at cfg3 (294 tiles,
    // ONE chunk of 128 planes each).)
    int zc = best_z_chunk(Di, nbx * nby, 2 * (long)cus, (Di + 3) / 4, 1.5);
    if (zc < 4) zc = 4;
    if (zc > Di) zc = Di;
    // the split-operand kernel addresses the skip tensor through a buffer descriptor (32-bit byte offsets);
    // MVS_TAIL_SPLIT=0: the fp32-MFMA form of the fused tail (conv11_prob_priv_kernel)
    const Form f = dtype != MVS_F32 ? kTail16
                 : opt.tail_split && (size_t)Di * Hi * Wi * 256 < k2_32 ? kTailSplit : kTailPriv;
    return marched(f, (int)nbx, (int)nby, z_split(Di, zc, nbx * nby));
}
// MVS_FUSE_PROB=0: conv11 and prob as two launches (A/B runs).  16-bit storage: the fused kernel runs the transposed
// convolution on the 16-bit matrix cores, so it stands in for the 16-bit MFMA layer kernels only (MVS_MFMA16=0 = fp32
// arithmetic on the narrowed operands: two launches)
inline bool tail_fused(int dtype, const Options& opt) { return opt.fuse_prob && (dtype == MVS_F32 || opt.mfma16); }
inline Plan plan_tail(int Di, int Hi, int Wi, int dtype, const Options& opt, int cus) {
    if (!tail_fused(dtype, opt)) return formed(kTailTwoLaunches);
    return plan_conv11_prob(Di, Hi, Wi, dtype, opt, cus);
}

// The tap-cache kernel needs 32-bit byte offsets into the feature copy and the volume, and o00 << 2 in an int; 2 <= N <= 5
// (16 VGPRs of cached taps per source view).  Other problems run the plain kernel.  fes / ves: bytes per feature / volume
// element.  (+ kMaxSlab + 4 depth planes of one channel plane: the parking range of the last block's out-of-image lanes)
inline bool warp_tc_fits(int N, int D, int h, int w, int fes, int ves) {
    const size_t hw = (size_t)h * w, park = kMaxSlab + 4;
    return N >= 2 && N <= 5 && 4 * (size_t)N * hw * 8 * fes < k2_31 &&
           4 * (size_t)D * hw * 8 * ves + park * hw * 8 * ves < k2_32 - 64 && hw < ((size_t)1 << 29);
}
// The warp + variance kernel of a problem whose feature copy has `fes` bytes per element (4, or 2 under MVS_FEAT16=1 in
// the 16-bit modes).  The tap-cache kernel is the default for fp32 features (2..5 views; MVS_WARP_TC=0 keeps the plain
// gather) and for 16-bit features too: cfg5 0.20 -> 0.15 ms, cfg3 1.84 -> 1.39 ms against the plain kernel
// (MVS_WARP_TC16=0 selects it; the FIRST form of the tap-cache kernel had been slower with 16-bit features).
inline Plan plan_warp(int N, int D, int h, int w, int dtype, int fes, const Options& opt) {
    const size_t hw = (size_t)h * w;
    // all views' features (N x 32 channels) against the 32 MB of aggregate L2
    const bool big = (size_t)N * hw * 32 * fes > ((size_t)24 << 20);
    if ((fes == 2 ? opt.warp_tc16 : opt.warp_tc) && warp_tc_fits(N, D, h, w, fes, dtype == MVS_F32 ? 4 : 2)) {
        // depths a thread marches through (cfg2, kernel + transpose: 8 / 12 / 16 / 24 / 32 / 48 / 64 = 0.183 / 0.172 / 0.168 /
        // 0.161 / 0.160 / 0.160 / 0.159 ms in round 3)
        // Round 4 sweep (bench per-kernel pass, cfg2 / cfg5 / cfg3): 12: 0.168 / 0.129 / 1.63; 20: 0.160 / 0.122 / 1.48; 24: 0.157
        // / 0.122 / 1.46; 28: 0.157 / 0.122 / 1.52; 40: 0.155 / 0.120 / 1.44; 52: 0.156 / 0.121 / 1.44; 88: 0.163 / 0.131 / 1.44
        // -- and a slab count that is a multiple of 8 is a trap in the depth-slab-fastest order (cfg3, D = 256: slab 16 /
        // 32 / 64 = 1.95 / 1.86 / 1.78 ms): the linear block id then sends slab s of EVERY pixel block to XCD s % 8, so every
        // XCD's L2 streams the whole feature set
        int slab = kTcSlabs[0];
        for (const int cand : kTcSlabs) {   // the first whose slab count is not a multiple of 8 (D = 320: 36)
            slab = cand;
            if (cdiv(D, cand) % 8 != 0) break;
        }
        const long npb = cdiv((long)hw, kTcPix);
        Plan p = marched(kWarpTc, (int)npb, 1, z_split(D, slab, npb));
        // MVS_WARP_DEPTH_FASTEST=1 / 0: always / never
        p.depth_fastest = opt.warp_depth_fastest_tc >= 0 ? opt.warp_depth_fastest_tc : (big ? 1 : 0);
        return p;
    }
    // MVS_WARP_DEPTH_FASTEST=1 forces the depth-slab-fastest block order (default: only when the feature maps exceed the
    // L2s), so tests can reach it at small shapes
    Plan p = formed(kWarpPlain);
    p.depth_fastest = opt.warp_depth_fastest || big;
    return p;
}

// ---- the test hook's query ----
enum { kQueryLayer = 0, kQueryTail = 1, kQueryWarp = 2 };
constexpr int kQueryInts = 9 + kNumOptions, kAnswerInts = 10;
// q = {which plan, layer, N, D, h, w, dtype, feature element size, CU count, the switches in Options' order};
// D, h, w are the dims of the planned launch's own input (a layer's Di, Hi, Wi; the tail's d9).
// a = {form, bz, by, bx, chunk size, chunk count, last chunk, grid, depth-fastest order, 1 where the form cuts along z}
inline int answer(const int* q, long long* a) {
    const int* v = q + 9;
    const Options opt{v[0] != 0, v[1] != 0, v[2] != 0, v[3] != 0, v[4] != 0, v[5] != 0, v[6] != 0, v[7] != 0, v[8] != 0, v[9] != 0,
                      v[10] != 0, v[11] != 0, v[12], v[13], v[14], v[15], v[16], v[17], v[18] != 0, v[19]};
    if (q[3] < 1 || q[4] < 1 || q[5] < 1 || q[8] < 1) return MVS_ERR_BAD_SHAPE;
    Plan p;
    switch (q[0]) {
        case kQueryLayer: p = plan_layer(q[1], q[3], q[4], q[5], q[6], opt, q[8]); break;
        case kQueryTail: p = plan_tail(q[3], q[4], q[5], q[6], opt, q[8]); break;
        case kQueryWarp: p = plan_warp(q[2], q[3], q[4], q[5], q[6], q[7], opt); break;
        default: return MVS_ERR_BAD_SHAPE;
    }
    const long long out[kAnswerInts] = {p.form, p.bz, p.by, p.bx, p.z.zc, p.z.n, p.z.last, p.z.grid, p.depth_fastest, p.z.n > 0};
    for (int i = 0; i < kAnswerInts; ++i) a[i] = out[i];
    return MVS_OK;
}

}  // namespace plan
}  // namespace mvs

// For the tests only, not part of the ABI (no header under include/ declares it) and free to change with the planner:
// plan::answer() on `query` (kQueryInts ints) into `answer` (kAnswerInts values).  Reads no environment variable and
// makes no HIP call, so it answers the same with and without a device.
extern "C" int mvs_test_launch_plan(const int* query, long long* answer);
