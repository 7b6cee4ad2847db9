"""The kernel-level parity entry points ("doors", csrc/op_door.hip.h) on the device: what their shared scaffold -- sizes, strides, uploads,
optional buffers, output fills -- could get wrong, at the smallest sizes that still cross each kernel's own tile once.  Every door with
B = 3 items of lengths {its minimum, a middle value, the whole row}:

  a. item independence: with NaN in the inputs at and beyond each length, item b of the batch is bit-equal to the call with that item
     alone and zeros there (the headers' "item b from x[b, :lengths[b]] only");
  b. a call with an optional output or input null leaves the other results bit-equal to the call with it present;
  c. two identical calls are bit-equal, and no output holds NaN (every door defines its whole output: zeros beyond an item's end).

The mono couple door is not in the table of check a: its kernel copies rows [0, C) of u * s into z on every column, those at and beyond
lengths[b] included (tests/test_mono_flows_gpu.py: "the x0 half passes through everywhere"), so NaN there comes back, before and after
the doors shared a scope.  include/vits_mi355_debug.h promises zeros; which of the two is right is the kernel's matter, not this file's.

The comparisons are of bytes: no tolerance.  DOORS is also what the one-off hash job of profiles/op_doors_identity.txt runs."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = ctypes.POINTER(ctypes.c_float)
I64 = ctypes.POINTER(ctypes.c_int64)
I32 = ctypes.POINTER(ctypes.c_int32)
i32 = ctypes.c_int32

LIMIT_TILE, PITCH_FRAME, GATING_BLOCK_16K = 2048, 1024, 6400
N_LIMIT = 2 * LIMIT_TILE + 37         # just over two VITS_LIMIT_TILE
N_PITCH = 3 * PITCH_FRAME + 77        # a few VITS_PITCH_FRAME
N_LOUD = GATING_BLOCK_16K + 137       # just over one 400 ms gating block at 16 kHz (and more than two limiter tiles)
N_SMALL = 333                         # resample, denoise: more than one 256-sample tile
T_ATT = 40                            # attention, mono couple: more than one 16- / 32-column tile
LIM = (1, 0.5, 5.0, 50.0)             # sample peaks, ceiling, lookahead_ms, release_ms


def _ptr(a, typ=F):
    return None if a is None else a.ctypes.data_as(typ)


def _check(lib, rc):
    assert rc == 0, (rc, lib._fn("last_error")().decode())


class Door:
    """One door at one size.  ins: the arrays with a leading B axis, whose last axis runs along the item (MAS: see `beyond`); lens: its
    length arrays [B]; shared: inputs without a B axis; call(lib, ins, lens, shared, skip) -> the outputs, each with a leading B axis
    (None for an output index in `skip`, passed as null; "tables" in `skip`: ek / ev null); optional: {name: skip-set} of check b."""

    def __init__(self, name, ins, lens, call, shared=(), optional=None, beyond=None, independent=True):
        self.name, self.ins, self.lens, self.shared, self.call, self.independent = name, ins, lens, shared, call, independent
        self.optional = optional or {}
        self.beyond = beyond or (lambda a, b, lens: np.broadcast_to(np.arange(a.shape[-1]) >= lens[0][b], a.shape[1:]))

    def padded(self, value):
        """the inputs with `value` at and beyond each item's lengths"""
        out = [a.copy() for a in self.ins]
        for a in out:
            for b in range(a.shape[0]):
                a[b][self.beyond(a, b, self.lens)] = value
        return out

    def run(self, lib, ins=None, lens=None, skip=(), shared=None):
        return self.call(lib, self.padded(0.0) if ins is None else ins, self.lens if lens is None else lens,
                         self.shared if shared is None else shared, skip)


def _noise(seed, *shape):
    return (0.3 * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)


def _items(name, N, scalars, outs, lo=0, optional=None, shared=()):
    """a door over x [B, N] + lengths through its C entry point: vits_<name>(device, x, lengths, B, N, *shared, *scalars, *outputs)"""
    def call(lib, ins, lens, shared, skip):
        B = ins[0].shape[0]
        ys = [None if k in skip else np.full(s, np.nan, np.float32) for k, s in enumerate(outs(lib, B))]
        _check(lib, lib._fn(name)(0, _ptr(ins[0]), _ptr(lens[0], I64), B, N, *[_ptr(s) for s in shared], *scalars, *[_ptr(y) for y in ys]))
        return ys
    return Door(name, [_noise(len(name), 3, N)], [np.array([lo, (lo + N) // 2, N], np.int64)], call, shared, optional)


def _stretch_len(lib, N):
    P, Q = lib.pitch_plan(3.0)
    return 256 * (-(-(N // 256 + 2) * P // Q) - 1)


def _attention(name, C, nh, tables):
    def call(lib, ins, lens, shared, skip):
        B, _, T = ins[0].shape
        out = np.full((B, C, T), np.nan, np.float32)
        if name == "plain_attention":
            fn = lib.lib.vits_debug_plain_attention
            fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int, F, I64, i32, i32, i32, i32, F]
            _check(lib, fn(0, _ptr(ins[0]), _ptr(lens[0], I64), B, C, T, nh, _ptr(out)))
        else:
            fn = lib.lib.vits_debug_relpos_attention
            fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int, F, F, F, I64, i32, i32, i32, i32, i32, F]
            ek, ev = (None, None) if "tables" in skip else shared
            _check(lib, fn(0, _ptr(ins[0]), _ptr(ek), _ptr(ev), _ptr(lens[0], I64), B, C, T, nh, 4, _ptr(out)))
        return [out]
    dk = C // nh
    shared = ()
    if tables == "random":
        shared = (_noise(5, 9, dk), _noise(6, 9, dk))
    elif tables == "zero":  # the relative-position terms add exact zeros: the table-less call must give the same bytes
        shared = (np.zeros((9, dk), np.float32), np.zeros((9, dk), np.float32))
    return Door(f"{name}[{tables}]" if tables else name, [_noise(C, 3, 3 * C, T_ATT)], [np.array([0, T_ATT // 2, T_ATT], np.int64)], call, shared,
                {"ek, ev": {"tables"}} if tables == "zero" else None)


def _mono(mode, C=32):
    def call(lib, ins, lens, shared, skip):
        B, _, T = ins[0].shape
        z = np.full((B, 2 * C, T), np.nan, np.float32)
        fn = lib.lib.vits_debug_mono_couple
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int, F, F, F, F, I64, i32, i32, i32, i32, F]
        _check(lib, fn(0, _ptr(ins[0]), _ptr(ins[1]), _ptr(shared[0]), _ptr(shared[1]), _ptr(lens[0], I64), B, C, T, mode, _ptr(z)))
        return [z]
    return Door(f"mono_couple[mode {mode}]", [_noise(1, 3, C, T_ATT), _noise(2, 3, 2 * C, T_ATT)], [np.array([0, T_ATT // 2, T_ATT], np.int64)], call,
                (_noise(3, C, C), _noise(4, C)), independent=False)


def _mas():
    def call(lib, ins, lens, shared, skip):
        B, Ty, Tx = ins[0].shape
        paths = np.full((B, Ty, Tx), -7, np.int32)
        _check(lib, lib._fn("mas_maximum_path")(0, _ptr(ins[0]), _ptr(lens[0], I32), _ptr(lens[1], I32), B, Ty, Tx, _ptr(paths, I32)))
        return [paths]
    # a ragged 3-item case: full extents, t_x == t_y, one token
    return Door("mas_maximum_path", [_noise(9, 3, 17, 5)], [np.array([17, 4, 9], np.int32), np.array([5, 4, 1], np.int32)], call,
                beyond=lambda a, b, lens: (np.arange(a.shape[1]) >= lens[0][b])[:, None] | (np.arange(a.shape[2]) >= lens[1][b])[None, :])


DOORS = [
    _items("op_resample", N_SMALL, (22050, 16000), lambda lib, B: [(B, lib.out_samples(N_SMALL, 22050, 16000))]),
    _items("op_denoise", N_SMALL, (64, 1.0), lambda lib, B: [(B, 16 * (N_SMALL // 16))], lo=33, shared=(np.abs(_noise(8, 33)),)),
    _items("op_loudness", N_LOUD, (16000,), lambda lib, B: [(B,), (B,)], optional={"loudness": {0}, "peak": {1}}),
    _items("op_loudness_normalize", N_LOUD, (16000, 1, -23.0, 0.0), lambda lib, B: [(B, N_LOUD), (B,), (B,)], optional={"loudness": {1}, "gain": {2}}),
    _items("op_true_peak", N_LIMIT, (16000,), lambda lib, B: [(B,)]),
    _items("op_limit_gain", N_LIMIT, (16000,) + LIM + (2.0,), lambda lib, B: [(B, N_LIMIT)]),
    _items("op_limit", N_LIMIT, (16000,) + LIM + (2.0,), lambda lib, B: [(B, N_LIMIT), (B,)], optional={"reduction": {1}}),
    _items("op_loudness_limit", N_LOUD, (16000, -14.0) + LIM, lambda lib, B: [(B, N_LOUD), (B,), (B,), (B,)],
           optional={"loudness": {1}, "gain": {2}, "reduction": {3}, "loudness, gain, reduction": {1, 2, 3}}),
    _items("op_pitch_shift", N_PITCH, (3.0,), lambda lib, B: [(B, N_PITCH)]),
    _items("op_pitch_stretch", N_PITCH, (3.0,), lambda lib, B: [(B, _stretch_len(lib, N_PITCH))]),
    _items("op_pitch_shift_formant", N_PITCH, (3.0,), lambda lib, B: [(B, N_PITCH)]),
    _items("op_pitch_stretch_formant", N_PITCH, (3.0,), lambda lib, B: [(B, _stretch_len(lib, N_PITCH))]),
    _items("op_pitch_formant_gain", N_PITCH, (3.0,), lambda lib, B: [(B, N_PITCH // 256 + 3, PITCH_FRAME // 2 + 1)]),
    _attention("plain_attention", 32, 2, None),
    _attention("relpos_attention", 64, 2, "random"),
    _attention("relpos_attention", 64, 2, "zero"),
    _mono(0),
    _mono(1),
    _mas(),
]
IDS = [d.name for d in DOORS]


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def batch(hip_lib):
    """every door's outputs for its batch with zeros beyond the lengths: computed once, shared by the three checks, left unchanged"""
    return {d.name: d.run(hip_lib) for d in DOORS}


@pytest.mark.parametrize("door", [d for d in DOORS if d.independent], ids=[d.name for d in DOORS if d.independent])
def test_item_independence(hip_lib, batch, door):
    got = door.run(hip_lib, ins=door.padded(np.nan))
    zeros = door.padded(0.0)
    for b in range(3):
        solo = door.run(hip_lib, ins=[a[b:b + 1] for a in zeros], lens=[ln[b:b + 1] for ln in door.lens])
        for k, (g, s) in enumerate(zip(got, solo)):
            assert _same(g[b:b + 1], s), f"{door.name}: output {k} of item {b} in the batch differs from the item alone"
    for k, (g, z) in enumerate(zip(got, batch[door.name])):
        assert _same(g, z), f"{door.name}: output {k} depends on what lies beyond the lengths"


@pytest.mark.parametrize("door, what", [(d, w) for d in DOORS for w in d.optional], ids=[f"{d.name}-{w}" for d in DOORS for w in d.optional])
def test_optional_buffers(hip_lib, batch, door, what):
    skip = door.optional[what]
    got = door.run(hip_lib, skip=skip)
    for k, (g, full) in enumerate(zip(got, batch[door.name])):
        if k in skip:
            assert g is None
            continue
        assert _same(g, full), f"{door.name} without {what}: output {k} differs from the call with it"


@pytest.mark.parametrize("door", DOORS, ids=IDS)
def test_repeatable_and_defined(hip_lib, batch, door):
    again = door.run(hip_lib)
    for k, (a, first) in enumerate(zip(again, batch[door.name])):
        assert _same(a, first), f"{door.name}: output {k} of two identical calls differs"
        if a.dtype == np.float32:
            assert not np.isnan(a).any(), f"{door.name}: output {k} holds NaN"
        else:
            assert ((a == 0) | (a == 1)).all(), f"{door.name}: output {k} holds an element the kernel did not write"
