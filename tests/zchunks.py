"""The launch plans of the depth path, asked of the library, and the test shapes chosen from them.

csrc/launch_plan.h plans every launch: the kernel form of a layer, of the fused tail and of the warp, its tile, and how
the z-marching launchers and the tap-cache warp cut the volume.  `plan` asks it through the library's test hook
(mvs_test_launch_plan: no GPU, no environment); the form names and the switches with their defaults are read from the
header.  The launcher functions below ask for one launcher's split under the switch that forces its z-marching form, as
the GPU tests run it, and return a `Split`: the chunk (or slab) size, the chunk count, the last chunk's size and the
grid.  `cheapest_cases` then picks, for a launcher and a CU count, the cheapest volume (D, h, w) of every case category
the kernels treat differently: one chunk, the ragged last chunks after a loop unrolled by 3, odd chunks, a one-plane
last chunk.  tests/test_zchunks_host.py pins the plans on known values; tests/test_gpu_zchunks.py runs the chosen shapes
on the GPU.

A shape is always the full-resolution cost volume (D, h, w) of the network; each launcher sees its own layer's input:
conv0 (D, h, w), conv1 (D, h, w) -> (D/2, h/2, w/2), conv2 at D/2, conv3 (D/2) -> (D/4), conv11_prob's input d9 at
(D/2, h/2, w/2).
"""
import ctypes
import functools
import os
import re
import sys
from typing import NamedTuple

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:      # a test file run as a child script has only tests/ on its path
    sys.path.insert(0, REPO)

from scene_3dreconstruction_mvsnet_amd import _lib  # noqa: E402

MAX_VOXELS = 1 << 21    # largest D * h * w a test case may use (about 2 M voxels)
HEADER = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc", "launch_plan.h")
LAYER, TAIL, WARP = 0, 1, 2     # kQueryLayer, kQueryTail, kQueryWarp


class Split(NamedTuple):
    zc: int     # planes per z chunk (depths per slab)
    n: int      # number of chunks (slabs)
    last: int   # planes of the last chunk
    grid: int   # blocks launched


class Plan(NamedTuple):
    form: str               # launch_plan.h's Form without its "k": "ConvZ16", "TailSplit", "WarpTc", ...
    tile: tuple             # (bz, by, bx) M-tiles per block of the 16-bit tile kernels, else (0, 0, 0)
    split: Split            # all zero where the form does not cut along z
    depth_fastest: int      # the warps' block order
    cuts_z: bool


@functools.lru_cache(maxsize=None)
def _header():
    """(form names in enum order, switch names in Options' order, their defaults) from launch_plan.h."""
    with open(HEADER) as f:
        src = f.read()
    forms = re.findall(r"^\s+k(\w+)(?: = 0)?,", re.search(r"enum Form \{(.*?)\n\};", src, re.S).group(1), re.M)
    names = re.findall(r"^\s+(?:bool|int) (\w+);", re.search(r"struct Options \{(.*?)\n\};", src, re.S).group(1), re.M)
    values = re.search(r"return Options\{(.*?)\};", src).group(1).split(",")
    defaults = [{"true": 1, "false": 0}.get(v.strip(), v) for v in values]
    defaults = [int(v) for v in defaults]
    assert len(names) == len(defaults) == 20 and forms[0] == "None", (forms, names, defaults)
    return forms, names, defaults


@functools.lru_cache(maxsize=None)
def _hook():
    fn = ctypes.CDLL(_lib.LIB_PATH).mvs_test_launch_plan
    fn.restype = ctypes.c_int
    return fn, (ctypes.c_int * 29)(), (ctypes.c_longlong * 10)()


def _ask(query):
    fn, q, a = _hook()
    q[:] = query
    st = fn(q, a)
    assert st == 0, (st, query)
    return a


@functools.lru_cache(maxsize=None)
def _switch_values(switches):
    """Options' 20 values: the defaults but for `switches`, a tuple of (field name, value)."""
    _, names, defaults = _header()
    assert {n for n, _ in switches} <= set(names), switches
    return [int(dict(switches).get(n, d)) for n, d in zip(names, defaults)]


def plan(which, D, h, w, cus, *, layer=0, N=1, storage="f32", fes=4, **switches):
    """The plan of one launch on an input of D x h x w (the launch's own input dims), at `cus` CUs, under the default
    switches but for `switches` (Options' field names)."""
    a = _ask([which, layer, N, D, h, w, _lib.DTYPE_CODES[storage], fes, cus] + _switch_values(tuple(sorted(switches.items()))))
    return Plan(_header()[0][a[0]], (a[1], a[2], a[3]), Split(a[4], a[5], a[6], a[7]), a[8], bool(a[9]))


def switch_names():
    return _header()[1]


# ---------------------------------------------------------------- one launcher's split, its z-marching form forced
def _forced(form, which, layer, storage, D, h, w, cus, *switch):
    """The split of a launch if its plan has `form` (the launcher's z-marching form), else None."""
    a = _ask([which, layer, 1, D, h, w, _lib.DTYPE_CODES[storage], 4, cus] + _switch_values(switch))
    return Split(a[4], a[5], a[6], a[7]) if _header()[0][a[0]] == form else None


def conv11_prob(D, h, w, cus):
    """launch_conv11_prob on d9 = (D/2, h/2, w/2); the chunks count INPUT planes."""
    return _forced("TailSplit", TAIL, 9, "f32", D // 2, h // 2, w // 2, cus)


def conv1z(D, h, w, cus):
    """fp32 conv1 on (D, h, w) under MVS_CONV1Z=1; the chunks count OUTPUT planes, and `cus` stands for MVS_PERSIST_CUS
    where the test sets it."""
    return _forced("Conv1Z", LAYER, 1, "f32", D, h, w, cus, ("conv1z", 1))


def convz16_dims(layer, D, h, w):
    """(Di, Hi, Wi, S) of convz16's layer 1 / 2 / 3 in a volume (D, h, w)."""
    if layer == 1:
        return D, h, w, 2
    if layer == 2:
        return D // 2, h // 2, w // 2, 1
    return D // 2, h // 2, w // 2, 2


def convz16(layer, D, h, w, cus):
    """16-bit conv1 / conv2 / conv3 under MVS_CONVZ16=1; the chunks count OUTPUT planes; None where the tile kernel runs
    instead (fewer than 4 output planes)."""
    Di, Hi, Wi, _ = convz16_dims(layer, D, h, w)
    return _forced("ConvZ16", LAYER, layer, "bf16", Di, Hi, Wi, cus, ("convz16", 1))


def conv0z16(D, h, w, cus):
    """16-bit conv0 under MVS_CONV0Z16=1; None where the tile kernel runs instead (D < 8)."""
    return _forced("Conv0Z16", LAYER, 0, "bf16", D, h, w, cus, ("conv0z16", 1))


def tc_slab(D, h, w):
    """The tap-cache warp's depth slab and grid (pixel blocks x slabs, in either block order); no CU count enters."""
    p = plan(WARP, D, h, w, 256, N=5)
    assert p.form == "WarpTc", p
    return p.split


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
