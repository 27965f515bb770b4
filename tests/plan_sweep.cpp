// plan_sweep.cpp -- every plan of csrc/launch_plan.h at the ends of the ABI's shape domain, as a stand-alone host program:
// tests/test_zchunks_host.py builds it with the host compiler and the address and undefined-behaviour sanitizers and runs
// the binary.  Checks that no plan's arithmetic overflows (the sanitizer ends the program) and that every z split is sound:
// chunks of 1 .. zc planes that add up to the depth, a positive grid of chunks x columns within HIP's 2^31 - 1 blocks.
#include <cstdio>
#include <initializer_list>

#include "launch_plan.h"

using namespace mvs;

static long n_plans = 0, n_bad = 0;

static void check(const char* what, const plan::Plan& p, int dz, const int* q, bool ask_hook = true) {
    ++n_plans;
    long long a[plan::kAnswerInts];
    bool ok = !ask_hook || (plan::answer(q, a) == MVS_OK && a[0] == p.form && a[4] == p.z.zc && a[5] == p.z.n && a[7] == p.z.grid);
    if (p.z.n > 0) {
        const long cols = (long)p.nbx * p.nby;
        ok = ok && p.z.zc >= 1 && p.z.last >= 1 && p.z.last <= p.z.zc && (long)(p.z.n - 1) * p.z.zc + p.z.last == dz;
        ok = ok && cols > 0 && p.z.grid > 0 && p.z.grid == cols * p.z.n && p.z.grid < ((long)1 << 31);
    } else if (p.form == plan::kConvGPersist) {
        ok = ok && p.z.grid > 0 && p.z.grid < ((long)1 << 31);
    }
    if (!ok) {
        ++n_bad;
        std::printf("BAD %s: layer %d N %d dims %d %d %d dtype %d fes %d cus %d -> form %d zc %d n %d last %d grid %ld cols %d x %d\n",
                    what, q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], (int)p.form, p.z.zc, p.z.n, p.z.last, p.z.grid, p.nbx, p.nby);
    }
}

static void fill(int* q, int which, int layer, int N, int D, int h, int w, int dtype, int fes, int cus, const Options& o) {
    const int v[plan::kQueryInts] = {which, layer, N, D, h, w, dtype, fes, cus,
        o.conv0_wino, o.conv_wino, o.conv0_split, o.split_layers, o.mfma16, o.fuse_prob, o.tail_split, o.warp_tc, o.warp_tc16,
        o.force_direct, o.feat16, o.feat_split01, o.conv1z, o.convz16, o.conv0z16, o.deep_tiles, o.split_deconv, o.persist_cus,
        o.warp_depth_fastest, o.warp_depth_fastest_tc};
    for (int i = 0; i < plan::kQueryInts; ++i) q[i] = v[i];
}

int main() {
    const int kMaxV = (int)kMaxConvInputVoxels;   // 2^28 - 1
    // the switch sets: defaults, every z-marching form forced, every one off with the fp32-MFMA forms
    Options forced = default_options(), off = default_options();
    forced.conv1z = forced.convz16 = forced.conv0z16 = forced.deep_tiles = 1;
    off.conv1z = off.convz16 = off.conv0z16 = off.deep_tiles = 0;
    off.split_layers = off.conv0_split = off.tail_split = off.warp_tc = off.warp_tc16 = false;
    const Options sets[] = {default_options(), forced, off};
    const int dtypes[] = {MVS_F32, MVS_F16, MVS_BF16};
    const int ends[] = {1, 2, 7, 8, 1 << 10, (1 << 14) - 1, 1 << 14, 1 << 20, kMaxV - 1, kMaxV};
    int q[plan::kQueryInts];
    for (const int cus : {1, 4, 80, 256, 304, 1024})
        for (const Options& o : sets)
            for (const int D : ends)
                for (const int h : ends)
                    for (const int w : ends) {
                        if ((size_t)D * h > kMaxConvInputVoxels) continue;   // (so that the product below cannot wrap)
                        const size_t vox = (size_t)D * h * w;
                        // a search over 2^25 and more chunk counts (D at the domain's end) takes a second under the sanitizers:
                        // only at the largest CU count, with the z-marching forms forced, planned once
                        const bool deep_search = D > (1 << 20);
                        if (deep_search && (cus != 1024 || &o != &sets[1])) continue;
                        for (const int dt : dtypes) {
                            if (deep_search && dt == MVS_F16) continue;   // the same code as bf16
                            if (vox <= kMaxConvInputVoxels)
                                for (int layer = 0; layer < MVS_NUM_LAYERS; ++layer) {
                                    const LayerSpec& S = kLayers[layer];
                                    if (S.stride == 2 && S.kind == kConv && ((D | h | w) & 1)) continue;
                                    if (layer == 10 && (5 * (size_t)h + 9) * (size_t)w + 33 > kMaxProbHaloVoxels) continue;
                                    fill(q, plan::kQueryLayer, layer, 1, D, h, w, dt, 4, cus, o);
                                    const plan::Plan p = plan::plan_layer(layer, D, h, w, dt, o, cus);
                                    check("layer", p, plan::out_dim(D, S.stride), q, !deep_search);
                                }
                            if (vox * 64 < ((size_t)1 << 31)) {   // mvs_conv11_prob's domain
                                fill(q, plan::kQueryTail, 9, 1, D, h, w, dt, 4, cus, o);
                                check("tail", plan::plan_tail(D, h, w, dt, o, cus), D, q);
                            }
                        }
                    }
    // the longest search at every CU count, as the hook answers it: one column through the 16-bit conv0's z-marching form,
    // of the most planes that form takes (16 output bytes per voxel below 2^32 - 64)
    const int kMaxZ = kMaxV - 7;
    for (const int cus : {1, 4, 80, 256, 304, 1024}) {
        fill(q, plan::kQueryLayer, 0, 1, kMaxZ, 1, 1, MVS_BF16, 4, cus, forced);
        long long a[plan::kAnswerInts];
        plan::Plan p;
        if (plan::answer(q, a) == MVS_OK && a[0] == plan::kConv0Z16) {
            p.form = plan::kConv0Z16;
            p.nbx = p.nby = 1;
            p.z = plan::ZSplit{(int)a[4], (int)a[5], (int)a[6], (long)a[7]};
        }
        check("longest search", p, kMaxZ, q, false);
        if (p.form != plan::kConv0Z16) { ++n_bad; std::printf("BAD longest search at %d CUs: not the z-marching form\n", cus); }
    }
    // the warp: h * w up to kMaxPixels and D up to kMaxSoftargminD, further than check_dims lets a volume of 32 channels go
    const int pix_ends[] = {2, 3, 1 << 10, 46340, 46341};   // 46340 x 46341 <= kMaxPixels
    for (const Options& o : sets)
        for (const int N : {1, 2, 5, 6, 64})
            for (const int D : {1, 2, 8, 320, 2048, kMaxSoftargminD})
                for (const int h : pix_ends)
                    for (const int w : pix_ends)
                        for (const int dt : dtypes)
                            for (const int fes : {4, 2}) {
                                if ((size_t)h * w > kMaxPixels || (fes == 2 && dt == MVS_F32)) continue;
                                fill(q, plan::kQueryWarp, 0, N, D, h, w, dt, fes, 256, o);
                                check("warp", plan::plan_warp(N, D, h, w, dt, fes, o), D, q);
                            }
    std::printf("plan_sweep: %ld plans, %ld bad\n", n_plans, n_bad);
    return n_bad ? 1 : 0;
}
