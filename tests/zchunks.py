"""The launch geometry the z-marching launchers and the tap-cache warp pick at run time, restated in Python.

Five launchers choose how a volume is cut along z from its shape and, for four of them, from the device's CU count.
Each function below restates one of those searches line for line (the source lines are quoted in its docstring) and
returns a `Split`: the chunk (or slab) size, the chunk count, the last chunk's size and the grid the kernel launches.
`cheapest_cases` then picks, for a launcher and a CU count, the cheapest volume (D, h, w) of every case category the
kernels treat differently: one chunk, the ragged last chunks after a loop unrolled by 3, odd chunks, a one-plane last
chunk.  tests/test_zchunks_host.py pins the restatements on known values; tests/test_gpu_zchunks.py runs the chosen
shapes on the GPU.

A shape is always the full-resolution cost volume (D, h, w) of the network; each launcher sees its own layer's input:
conv0 (D, h, w), conv1 (D, h, w) -> (D/2, h/2, w/2), conv2 at D/2, conv3 (D/2) -> (D/4), conv11_prob's input d9 at
(D/2, h/2, w/2).
"""
import functools
from typing import NamedTuple

MAX_VOXELS = 1 << 21    # largest D * h * w a test case may use (about 2 M voxels)


class Split(NamedTuple):
    zc: int     # planes per z chunk (depths per slab)
    n: int      # number of chunks (slabs)
    last: int   # planes of the last chunk
    grid: int   # blocks launched


def _cdiv(a, b):
    return (a + b - 1) // b


def _best_split(dz, nb_per_chunk, slots, nz_max, prologue):
    """The search every z-marching launcher shares: the chunk count nz in 1..nz_max with the best fill of the last
    round of `slots` resident blocks, discounted by a per-chunk prologue of `prologue` steps; the first best wins."""
    best, best_eff = 1, 0.0
    for nz in range(1, nz_max + 1):
        zc = _cdiv(dz, nz)
        nzc = _cdiv(dz, zc)
        nb = nb_per_chunk * nzc
        eff = nb / (_cdiv(nb, slots) * slots) * zc / (zc + prologue)
        if eff > best_eff + 1e-9:
            best_eff, best = eff, nz
    return best


def _split(dz, zc, ncol):
    n = _cdiv(dz, zc)
    return Split(zc, n, dz - (n - 1) * zc, ncol * n)


@functools.lru_cache(maxsize=None)
def _conv11_prob_z(Di, ntile, cus):
    best = _best_split(Di, ntile, 2 * cus, (Di + 3) // 4, 1.5)
    ZC = min(max(_cdiv(Di, best), 4), Di)
    return _split(Di, ZC, ntile)


def conv11_prob(D, h, w, cus):
    """launch_conv11_prob (csrc/conv11_prob.hip), on d9 = (D/2, h/2, w/2); ZC counts INPUT planes:

        const int nbx = (Wo - 2 + PX - 1) / PX > 0 ? (Wo - 2 + PX - 1) / PX : 1;      // PX = 30, PY = 14
        const int ntile = nbx * nby, slots = 2 * cus;
        for (int nz = 1; nz <= (Di + 3) / 4; ++nz) { ... zc / (zc + 1.5) ... }
        int ZC = (Di + best - 1) / best;  if (ZC < 4) ZC = 4;  if (ZC > Di) ZC = Di;
        const dim3 grid(nbx * nby * nzc);
    """
    Di, Hi, Wi = D // 2, h // 2, w // 2
    nbx = max((2 * Wi - 2 + 29) // 30, 1)
    nby = max((2 * Hi - 2 + 13) // 14, 1)
    return _conv11_prob_z(Di, nbx * nby, cus)


@functools.lru_cache(maxsize=None)
def _conv1z_z(Do, ncol, cus):
    best = _best_split(Do, ncol, cus, (Do + 3) // 4, 2.5)
    return _split(Do, _cdiv(Do, best), ncol)


def conv1z(D, h, w, cus):
    """run_conv1z (csrc/conv3d_mfma.hip), fp32 conv1 on (D, h, w); ZC counts OUTPUT planes, and `cus` is
    persistent_blocks_per_cu_scale(): MVS_PERSIST_CUS if set, else device_cus():

        const int nbx = (Wo + TXO - 1) / TXO, nby = (Ho + TYO - 1) / TYO, ncol = nbx * nby;   // TXO = 16, TYO = 8
        for (int nz = 1; nz <= (Do + 3) / 4; ++nz) { ... zc / (zc + 2.5) ... }
        const int ZC = (Do + best - 1) / best, nzc = (Do + ZC - 1) / ZC;
        conv1z_mfma_kernel<<<ncol * nzc, THREADS, 0, s>>>
    """
    Do, Ho, Wo = (D - 1) // 2 + 1, (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return _conv1z_z(Do, _cdiv(Wo, 16) * _cdiv(Ho, 8), cus)


def convz16_dims(layer, D, h, w):
    """(Di, Hi, Wi, S) of convz16's layer 1 / 2 / 3 in a volume (D, h, w)."""
    if layer == 1:
        return D, h, w, 2
    if layer == 2:
        return D // 2, h // 2, w // 2, 1
    return D // 2, h // 2, w // 2, 2


def convz16(layer, D, h, w, cus):
    """run_convz16 (csrc/conv3d_mfma16.hip), 16-bit conv1 / conv2 / conv3 (MVS_CONVZ16=1); ZC counts OUTPUT planes and
    `cus` is device_cus() (try_convz16); None where try_convz16 leaves the layer to the tile kernel:

        static constexpr int TY = 8, TX = (S == 1) ? 32 : 16;      // ConvZ16
        const int nbx = (Wo + G::TX - 1) / G::TX, nby = (Ho + G::TY - 1) / G::TY, ncol = nbx * nby;
        for (int nz = 1; nz <= (Do + 3) / 4; ++nz) { ... zc / (zc + 2.5) ... }
        const int ZC = (Do + best - 1) / best, nzc = (Do + ZC - 1) / ZC;
        convz16_mfma_kernel<DT, CIN, COUT, S><<<ncol * nzc, G::THREADS, 0, s>>>
    """
    Di, Hi, Wi, S = convz16_dims(layer, D, h, w)
    Do, Ho, Wo = (Di - 1) // S + 1, (Hi - 1) // S + 1, (Wi - 1) // S + 1
    if Do < 4:   # try_convz16: `|| Do < 4) return MVS_OK;` -- the tile kernel runs instead
        return None
    tx = 32 if S == 1 else 16
    return _conv1z_z(Do, _cdiv(Wo, tx) * _cdiv(Ho, 8), cus)   # the same search as run_conv1z


C0Z_TY = 8   # c0z::TY (C0Z_TY in conv3d_mfma16.hip): rows and waves per block


@functools.lru_cache(maxsize=None)
def _conv0z16_z(Di, ncol, cus):
    best = _best_split(Di, ncol, cus * (8 // C0Z_TY), Di // 8, 2.0)
    return _split(Di, _cdiv(Di, best), ncol)


def conv0z16(D, h, w, cus):
    """The conv0z16 branch of launch_layer16_dt (csrc/conv3d_mfma16.hip), 16-bit conv0 (MVS_CONV0Z16=1); None where
    the branch is not taken:

        const int ncol = ((Wi + c0z::TX - 1) / c0z::TX) * ((Hi + c0z::TY - 1) / c0z::TY);     // TX = 32, TY = 8
        for (int nz = 1; nz <= Di / 8; ++nz) { ... slots = (long)cus * (8 / c0z::TY); ... zc / (zc + 2.0) ... }
        const int ZC = (Di + best - 1) / best, nzc = (Di + ZC - 1) / ZC;
        conv0z16_mfma_kernel<DT><<<ncol * nzc, c0z::THREADS, 0, s>>>
    """
    if D < 8:   # `zmarch != 0 && Di >= 8 && ...`: the tile kernel runs instead
        return None
    return _conv0z16_z(D, _cdiv(w, 32) * _cdiv(h, C0Z_TY), cus)


TC_SLABS = (40, 44, 36, 32, 28, 24)
TC_PIX = 32   # pixels per block: 256 threads / 8 lanes per pixel (CPT = 4)


def tc_slab(D, h, w):
    """launch_tc2_dt (csrc/warp_variance_tc.hip): the depth slab and the grid (npb pixel blocks x nsl slabs, in
    either block order); no CU count enters:

        for (const int cand : {40, 44, 36, 32, 28, 24}) { slab = cand; if (((D + cand - 1) / cand) % 8 != 0) break; }
        const unsigned npb = (h * w + pix - 1) / pix, nsl = (D + slab - 1) / slab;
    """
    slab = TC_SLABS[0]
    for cand in TC_SLABS:
        slab = cand
        if _cdiv(D, cand) % 8 != 0:
            break
    return _split(D, slab, _cdiv(h * w, TC_PIX))


# ---------------------------------------------------------------- the launchers and their case categories
LAUNCHERS = {
    "conv11_prob": conv11_prob,
    "conv1z": conv1z,
    "convz16-1": functools.partial(convz16, 1),
    "convz16-2": functools.partial(convz16, 2),
    "convz16-3": functools.partial(convz16, 3),
    "conv0z16": conv0z16,
}


def categories(name, s):
    """The case categories a split falls in.  "single": one chunk.  "zcA-lastB": a ragged last chunk (last < ZC) with
    ZC = A and last = B mod 3 (the loops unrolled by 3 leave one or two steps over at B = 1, 2).  conv11_prob also:
    "odd-zc" (a chunk ends on an odd input plane, so its last conv11 plane pairs with the next chunk's first) and
    "last1" (a last chunk of one input plane)."""
    out = []
    if s is None:
        return out
    if s.n == 1:
        out.append("single")
    elif s.last < s.zc:
        out.append(f"zc{s.zc % 3}-last{s.last % 3}")
    if name == "conv11_prob" and s.n > 1:
        if s.zc % 2 == 1:
            out.append("odd-zc")
        if s.last == 1:
            out.append("last1")
    return out


def required_categories(name):
    """Categories every CU count must reach within MAX_VOXELS: one chunk, and a ragged last chunk of 1 or 2 planes
    mod 3 after chunks of 0, 1 and 2 planes mod 3; for conv11_prob an odd ZC and a one-plane last chunk."""
    req = ["single"] + [f"zc{a}-last{b}" for a in range(3) for b in (1, 2)]
    if name == "conv11_prob":
        req += ["odd-zc", "last1"]
    return req


@functools.lru_cache(maxsize=None)
def _shapes_by_cost():
    """Every (D, h, w) with multiples of 8 and D * h * w <= MAX_VOXELS, cheapest first (ties: smaller D, h)."""
    out = []
    for D in range(8, MAX_VOXELS // 64 + 1, 8):
        for h in range(8, MAX_VOXELS // (8 * D) + 1, 8):
            for w in range(8, MAX_VOXELS // (D * h) + 1, 8):
                out.append((D * h * w, D, h, w))
    out.sort()
    return tuple(s[1:] for s in out)


@functools.lru_cache(maxsize=None)
def cheapest_cases(name, cus, min_zc=0):
    """{category: (D, h, w)}: the cheapest shape of every category `name` reaches at `cus` CUs, among the splits with
    chunks of at least `min_zc` planes."""
    fn = LAUNCHERS[name]
    found = {}
    for shape in _shapes_by_cost():
        s = fn(*shape, cus)
        if s is None or s.zc < min_zc:
            continue
        for cat in categories(name, s):
            found.setdefault(cat, shape)
    return found
