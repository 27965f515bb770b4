"""The guarded arena (tests/guarded.py) has teeth: on CPU tensors, with small torch functions standing in for kernels,
every emulated defect is reported and the correct stand-ins pass."""
import itertools
import types

import pytest
import torch

import guarded as G

D, H, W = 5, 7, 9            # a ragged little volume: one z-plane is 63 floats
TILE = 4                      # rows per "tile" of the stand-in: the last tile has 3 rows


def _x():
    return torch.arange(D * H * W, dtype=torch.float32).reshape(D, H, W) / 7 - 11


def _flat_after(arena, t, n):
    """n elements of t's dtype right behind t (the stand-in's out-of-bounds store target)."""
    r = arena.record(t)
    return arena.block[r.end:r.end + n * t.element_size()].view(t.dtype)


def _flat_before(arena, t, n):
    r = arena.record(t)
    return arena.block[r.start - n * t.element_size():r.start].view(t.dtype)


def scale_kernel(arena, defect=None):
    """y = 2 x, tile by tile over the rows, with a one-element scratch that a correct kernel writes before it reads."""
    x = arena.put(_x(), "in", "x")
    y = arena.carve((D, H, W), torch.float32, "out", "y")
    ws = arena.carve((16,), torch.float32, "scratch", "ws")
    if defect == "last_element":
        y.view(-1)[:-1] = 2 * x.view(-1)[:-1]
    else:
        rows = H - 1 if defect == "last_row" else H   # the last tile's last row of every plane
        for r0 in range(0, rows, TILE):
            y[:, r0:min(r0 + TILE, rows)] = 2 * x[:, r0:min(r0 + TILE, rows)]
    if defect == "store_after":
        _flat_after(arena, y, 1)[0] = 1.0
    elif defect == "store_before":
        _flat_before(arena, y, 1)[0] = 1.0
    elif defect == "plane_after":
        _flat_after(arena, y, H * W)[:] = 2 * x[-1].reshape(-1)
    elif defect == "scratch_times_zero":
        y[0, 0, 0] = y[0, 0, 0] + 0.0 * ws[3]
    elif defect == "scratch_added":
        y[0, 0, 0] = y[0, 0, 0] + ws[3]
    elif defect == "scratch_added_if_finite":      # NaN-proof, so 0xFF passes: only 0x4B against 0x00 shows it
        y[0, 0, 0] = y[0, 0, 0] + torch.nan_to_num(ws[3], nan=0.0)
    elif defect == "input_modified":
        x[1, 2, 3] += 1.0
    else:
        ws[3] = 5.0
        y[0, 0, 0] = y[0, 0, 0] + 0.0 * ws[3]      # written first: a legitimate scratch use
    return y


def test_clean_stand_in_passes_and_matches_the_plain_result():
    arena = G.Arena(1 << 20)
    got, guard_bytes = G.same_under_all_poisons(arena, scale_kernel)
    G.assert_same_bytes(got, [2 * _x()])
    assert guard_bytes >= 6 * G.MIN_GUARD


@pytest.mark.parametrize("defect,words", [
    ("last_element", "depends on what its buffers held"),
    ("last_row", "depends on what its buffers held"),
    ("store_after", "guard after y"),
    ("store_before", "guard before y"),
    ("plane_after", "guard after y"),
    ("scratch_times_zero", "depends on what its buffers held"),
    ("scratch_added", "depends on what its buffers held"),
    ("scratch_added_if_finite", "0x00 and 0x4B"),
    ("input_modified", "input x"),
])
def test_emulated_defect_is_reported(defect, words):
    arena = G.Arena(1 << 20)
    with pytest.raises(AssertionError, match=words):
        G.same_under_all_poisons(arena, lambda a: scale_kernel(a, defect))


def test_reports_name_the_tensor_the_side_and_the_first_offset():
    arena = G.Arena(1 << 20)
    arena.reset(poison=0xFF)
    y = scale_kernel(arena, "store_after")
    (msg,) = arena.check()
    assert "guard after y" in msg and "first at offset 0 " in msg and "4 bytes changed" in msg
    arena.reset(poison=0xFF)
    y = scale_kernel(arena, "store_before")
    (msg,) = arena.check()
    assert "guard before y" in msg and "first at offset -4 " in msg
    arena.reset()
    y = scale_kernel(arena, "input_modified")
    (msg,) = arena.check()
    first = int(msg.rsplit("first at byte ", 1)[1])
    assert msg.startswith("input x") and first // 4 == (1 * H + 2) * W + 3
    del y


def test_a_whole_plane_past_the_end_stays_inside_the_guard():
    """The guard is as wide as one outermost slice even where that exceeds 64 KiB: a z-plane stored past the end of a
    big-plane volume changes guard bytes only."""
    h, w = 130, 140                                   # one fp32 plane = 72,800 bytes > MIN_GUARD
    arena = G.Arena(4 << 20)
    y = arena.carve((3, h, w), torch.float32, "out", "vol")
    nb = arena.carve((8,), torch.float32, "in", "neighbour")
    r = arena.record(y)
    assert r.hi - r.end >= h * w * 4 > G.MIN_GUARD and r.start - r.lo >= h * w * 4
    before = G.raw_bytes(nb).clone()
    _flat_after(arena, y, h * w)[:] = 1.0
    (msg,) = arena.check()
    assert "guard after vol" in msg and f"{h * w * 4} bytes changed" in msg
    assert torch.equal(G.raw_bytes(nb), before)


def test_inout_and_in_buffers_are_never_poisoned():
    arena = G.Arena(1 << 20)
    acc = arena.put(torch.ones(8, dtype=torch.float64), "inout", "sums")
    x = arena.put(torch.ones(8), "in", "x")
    for t in (acc, x):
        with pytest.raises(ValueError, match="only 'out' and 'scratch'"):
            arena.poison_one(t)
    assert bool((acc == 1).all()) and bool((x == 1).all())
    with pytest.raises(ValueError):
        arena.put(torch.ones(8), "out")
    acc += 1                                         # an in-place update of an inout buffer is no finding
    assert arena.check() == []


def test_guard_and_poisons_differ_in_every_byte_and_mean_what_the_module_says():
    for a, b in itertools.combinations((G.GUARD,) + G.POISONS, 2):
        assert 0 <= a <= 255 and 0 <= b <= 255 and a != b      # one-byte patterns: every byte of a fill differs
    ff = torch.full((8,), 0xFF, dtype=torch.uint8)
    for dt in (torch.float32, torch.float16, torch.bfloat16, torch.float64):
        assert bool(torch.isnan(ff.view(dt)).all())
    assert int(ff.view(torch.int32)[0]) == -1
    kb = torch.full((8,), 0x4B, dtype=torch.uint8)
    assert 1.2e7 < float(kb.view(torch.float32)[0]) < 1.4e7
    assert 1.2e7 < float(kb.view(torch.bfloat16)[0]) < 1.4e7
    assert 14.5 < float(kb.view(torch.float16)[0]) < 14.7
    assert G.MIN_GUARD == 64 * 1024 and G.ALIGN == 256


def test_carved_views_are_aligned_poisoned_and_fenced():
    arena = G.Arena(2 << 20)
    for p in G.POISONS:
        arena.reset(poison=p)
        ts = [arena.carve(s, dt, role) for s, dt, role in (((3, 5, 7), torch.float32, "out"), ((13,), torch.uint8, "scratch"),
                                                           ((2, 9), torch.float16, "out"), ((5,), torch.float64, "out"),
                                                           ((1, 3, 3), torch.bfloat16, "scratch"))]
        for t in ts:
            r = arena.record(t)
            assert t.data_ptr() % G.ALIGN == 0 and t.is_contiguous()
            assert bool((G.raw_bytes(t) == p).all())
            assert r.start - r.lo >= G.MIN_GUARD and r.hi - r.end >= G.MIN_GUARD
            assert bool((arena.block[r.lo:r.start] == G.GUARD).all()) and bool((arena.block[r.end:r.hi] == G.GUARD).all())
        spans = [(arena.record(t).lo, arena.record(t).hi) for t in ts]
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    with pytest.raises(MemoryError):
        arena.carve((4 << 20,), torch.uint8, "scratch")
    with pytest.raises(ValueError):
        arena.reset(poison=0x11)


def test_intercept_carves_a_modules_own_allocations():
    """The proxy replaces the name `torch` in a module: its `empty` / `empty_like` come from the arena with a role, other
    devices and everything else are torch's own, and the name is restored afterwards."""
    mod = types.ModuleType("standin")
    mod.torch = torch
    exec("def f(x):\n"
         "    ws = torch.empty(32, dtype=torch.uint8, device=x.device)\n"
         "    y = torch.empty((2, 3), dtype=torch.float32, device=x.device)\n"
         "    z = torch.empty_like(y)\n"
         "    host = torch.empty(4, dtype=torch.uint8, device='meta')\n"
         "    y.copy_(x); z.copy_(torch.flip(x, (0,)))\n"
         "    return ws, y, z, host\n", mod.__dict__)
    arena = G.Arena(1 << 20)
    arena.reset(poison=0x4B)
    x = arena.put(torch.arange(6.0).reshape(2, 3), "in")
    with arena.intercept(mod):
        ws, y, z, host = mod.f(x)
    assert mod.torch is torch
    assert [r.role for r in arena.carved] == ["in", "scratch", "out", "out"]
    assert arena.record(ws).role == "scratch" and host.device.type == "meta"
    assert bool((ws == 0x4B).all()) and torch.equal(y, x) and torch.equal(z, torch.flip(x, (0,)))
    assert arena.check() == []


def test_an_allocation_the_proxy_cannot_carve_fails_the_block():
    """A wrapper that allocates its output another way (torch.zeros, keywords, a non-contiguous empty_like) would run
    unpoisoned and unguarded: leaving the intercepted block reports it, and so does an output outside the arena."""
    mod = types.ModuleType("standin")
    mod.torch = torch
    exec("def zeros(x):\n    return torch.zeros((2, 3), dtype=torch.float32, device=x.device)\n"
         "def pinned(x):\n    return torch.empty((2, 3), dtype=torch.float32, device=x.device, requires_grad=False)\n"
         "def like(x):\n    return torch.empty_like(x.t())\n"
         "def new(x):\n    return x.new_empty((2, 3)).copy_(x)\n", mod.__dict__)
    arena = G.Arena(1 << 20)
    for name in ("zeros", "pinned", "like"):
        arena.reset()
        x = arena.put(torch.arange(6.0).reshape(2, 3), "in")
        with pytest.raises(AssertionError, match="allocated outside the arena"):
            with arena.intercept(mod):
                getattr(mod, name)(x)
        assert mod.torch is torch

    def fn(a):
        x = a.put(torch.arange(6.0).reshape(2, 3), "in")
        with a.intercept(mod):
            return mod.new(x)
    with pytest.raises(AssertionError, match="output 0 .* was not carved from the arena"):
        G.same_under_all_poisons(arena, fn)
    arena.reset()
    y = arena.carve((4, 3), torch.float32, "out", "y")
    assert arena.owner(y[1:3]).name == "y" and arena.owner(y).name == "y"
    with pytest.raises(KeyError):
        arena.owner(torch.empty(3))
