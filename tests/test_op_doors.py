"""The kernel-level parity entry points ("doors", csrc/op_door.hip.h), the part that needs no GPU: what each door refuses before its first
HIP call, with the code and the vits_last_error text, and the two host-only identity paths.  The C doors are called directly
(hip_lib._fn), so that the Python wrappers' own checks do not get there first.

EXPECTED was recorded from the library as it stood before the doors shared one scope.  Two things differ from that record, on purpose:
the length refusals of the resample, plain attention, relpos attention and mono couple doors name the item and the value (they said
"<door>: length out of range"), and the clock probe's error is negative, as include/vits_mi355_debug.h documents (it was +1).

Not in the table, because the call is not refused and goes on to the device: B = 65536 for the MAS and conv1d doors (they have no
upper bound on B), and a null output for vits_op_loudness (both of its outputs are optional)."""
import ctypes

import numpy as np
import pytest

from vosk_tts_amd.capi import VitsError

F = ctypes.POINTER(ctypes.c_float)
I64 = ctypes.POINTER(ctypes.c_int64)
I32 = ctypes.POINTER(ctypes.c_int32)
i32 = ctypes.c_int32

B0, N0 = 3, 512
X = np.zeros((B0, N0), np.float32)
OUT = [np.zeros((B0, N0), np.float32) for _ in range(4)]
BIAS = np.zeros(33, np.float32)  # filter_length 64
LIM = (1, 0.5, 5.0, 50.0)        # mode, ceiling, lookahead_ms, release_ms

# door -> (the scalars between N and the outputs, number of outputs, the smallest valid length, whether a null first output is refused)
ITEM_DOORS = {
    "op_resample": ((16000, 8000), 1, 0, True),
    "op_denoise": ((BIAS.ctypes.data_as(F), 64, 1.0), 1, 33, True),
    "op_loudness": ((16000,), 2, 0, False),
    "op_loudness_normalize": ((16000, 1, -23.0, 0.0), 3, 0, True),
    "op_true_peak": ((16000,), 1, 0, True),
    "op_limit_gain": ((16000,) + LIM + (1.0,), 1, 0, True),
    "op_limit": ((16000,) + LIM + (1.0,), 2, 0, True),
    "op_loudness_limit": ((16000, -23.0) + LIM, 4, 0, True),
    "op_pitch_shift": ((3.0,), 1, 0, True),
    "op_pitch_stretch": ((3.0,), 1, 0, True),
    "op_pitch_shift_formant": ((3.0,), 1, 0, True),
    "op_pitch_stretch_formant": ((3.0,), 1, 0, True),
    "op_pitch_formant_gain": ((3.0,), 1, 0, True),
}


def _ptr(a, typ=F):
    return None if a is None else a.ctypes.data_as(typ)


NULL = "null"


def _item_call(door, x=X, lengths=None, B=B0, N=N0, scalars=None, null_out=False):
    sc, n_out, lo, _ = ITEM_DOORS[door]
    ln = None if lengths is NULL else _lens(N0, lo) if lengths is None else lengths
    outs = [_ptr(o) for o in OUT[:n_out]]
    if null_out:
        outs[0] = None
    return lambda lib: lib._fn(door)(0, _ptr(x), _ptr(ln, I64), B, N, *(sc if scalars is None else scalars), *outs)


def _lens(last, lo=0):
    return np.array([lo, 100, last], np.int64)


def _debug_fn(lib, name, argtypes):
    fn = getattr(lib.lib, "vits_debug_" + name)
    fn.restype = ctypes.c_int
    fn.argtypes = argtypes
    return fn


C0, T0 = 64, 40
QKV = np.zeros((B0, 3 * C0, T0), np.float32)
TAB = np.zeros((9, 32), np.float32)
LEN_T = np.array([0, 20, T0], np.int64)
OUT_T = np.zeros((B0, 2 * C0, T0), np.float32)
H = np.zeros((B0, C0, T0), np.float32)
WM = np.zeros((C0, C0), np.float32)


def _plain(qkv=QKV, lengths=LEN_T, B=B0, C=C0, T=T0, nh=2, out=OUT_T):
    def call(lib):
        fn = _debug_fn(lib, "plain_attention", [ctypes.c_int, F, I64, i32, i32, i32, i32, F])
        return fn(0, _ptr(qkv), _ptr(lengths, I64), B, C, T, nh, _ptr(out))
    return call


def _relpos(qkv=QKV, ek=TAB, ev=TAB, lengths=LEN_T, B=B0, C=C0, T=T0, nh=2, window=4, out=OUT_T):
    def call(lib):
        fn = _debug_fn(lib, "relpos_attention", [ctypes.c_int, F, F, F, I64, i32, i32, i32, i32, i32, F])
        return fn(0, _ptr(qkv), _ptr(ek), _ptr(ev), _ptr(lengths, I64), B, C, T, nh, window, _ptr(out))
    return call


def _mono(h=H, u=OUT_T, W=WM, b=BIAS, lengths=LEN_T, B=B0, C=C0, T=T0, mode=0, z=OUT_T):
    def call(lib):
        fn = _debug_fn(lib, "mono_couple", [ctypes.c_int, F, F, F, F, I64, i32, i32, i32, i32, F])
        return fn(0, _ptr(h), _ptr(u), _ptr(W), _ptr(b), _ptr(lengths, I64), B, C, T, mode, _ptr(z))
    return call


TY0, TX0 = 6, 4
VAL = np.zeros((B0, TY0, TX0), np.float32)
PATHS = np.zeros((B0, TY0, TX0), np.int32)
EXT_Y = np.array([TY0, 5, 4], np.int32)
EXT_X = np.array([TX0, 3, 2], np.int32)


def _mas(values=VAL, t_ys=EXT_Y, t_xs=EXT_X, B=B0, Ty=TY0, Tx=TX0, paths=PATHS):
    return lambda lib: lib._fn("mas_maximum_path")(0, _ptr(values), _ptr(t_ys, I32), _ptr(t_xs, I32), B, Ty, Tx, _ptr(paths, I32))


def _conv(x=X, w=X, bias=None, B=1, Cin=16, Cout=16, T=8, K=3, dil=1, y=OUT[0]):
    return lambda lib: lib._fn("op_conv1d")(0, _ptr(x), _ptr(w), _ptr(bias), B, Cin, Cout, T, K, dil, 0.1, _ptr(y))


def _bad_calls():
    c = {}
    for door, (_, _, lo, null_out_refused) in ITEM_DOORS.items():
        c[f"{door}-null_x"] = _item_call(door, x=None)
        c[f"{door}-null_lengths"] = _item_call(door, lengths=NULL)
        if null_out_refused:
            c[f"{door}-null_out"] = _item_call(door, null_out=True)
        c[f"{door}-B_0"] = _item_call(door, B=0)
        c[f"{door}-B_65536"] = _item_call(door, B=65536)
        c[f"{door}-N_0"] = _item_call(door, N=0)
        c[f"{door}-N_2^31"] = _item_call(door, N=1 << 31)
        c[f"{door}-len_-1"] = _item_call(door, lengths=_lens(-1, lo))
        c[f"{door}-len_N+1"] = _item_call(door, lengths=_lens(N0 + 1, lo))
    c["op_denoise-null_bias"] = _item_call("op_denoise", scalars=(None, 64, 1.0))
    c["op_denoise-len_below_half_filter"] = _item_call("op_denoise", lengths=_lens(32, 33))
    c["op_pitch_stretch-identity"] = _item_call("op_pitch_stretch", scalars=(0.0,))
    c["op_pitch_stretch_formant-identity"] = _item_call("op_pitch_stretch_formant", scalars=(0.0,))
    c["op_pitch_formant_gain-identity"] = _item_call("op_pitch_formant_gain", scalars=(0.0,))

    for name, f in (("plain_attention", _plain), ("relpos_attention", _relpos)):
        c[f"{name}-null_qkv"] = f(qkv=None)
        c[f"{name}-null_lengths"] = f(lengths=None)
        c[f"{name}-null_out"] = f(out=None)
        c[f"{name}-B_0"] = f(B=0)
        c[f"{name}-B_65536"] = f(B=65536)
        c[f"{name}-T_0"] = f(T=0)
        c[f"{name}-C_not_a_multiple_of_heads"] = f(C=65)
        c[f"{name}-len_-1"] = f(lengths=np.array([0, 20, -1], np.int64))
        c[f"{name}-len_T+1"] = f(lengths=np.array([0, 20, T0 + 1], np.int64))
    c["plain_attention-head_dim_40"] = _plain(C=80)
    c["relpos_attention-ek_only"] = _relpos(ev=None)
    c["relpos_attention-ev_only"] = _relpos(ek=None)
    c["relpos_attention-head_dim_16"] = _relpos(C=32)
    c["relpos_attention-window_5"] = _relpos(window=5)

    for arg in ("h", "u", "W", "b", "lengths", "z"):
        c[f"mono_couple-null_{arg}"] = _mono(**{arg: None})
    c["mono_couple-B_0"] = _mono(B=0)
    c["mono_couple-B_65536"] = _mono(B=65536)
    c["mono_couple-T_0"] = _mono(T=0)
    c["mono_couple-C_48"] = _mono(C=48)
    c["mono_couple-mode_2"] = _mono(mode=2)
    c["mono_couple-len_-1"] = _mono(lengths=np.array([0, 20, -1], np.int64))
    c["mono_couple-len_T+1"] = _mono(lengths=np.array([0, 20, T0 + 1], np.int64))

    for arg in ("values", "t_ys", "t_xs", "paths"):
        c[f"mas-null_{arg}"] = _mas(**{arg: None})
    c["mas-B_0"] = _mas(B=0)
    c["mas-Ty_0"] = _mas(Ty=0)
    c["mas-Tx_0"] = _mas(Tx=0)
    c["mas-t_y_-1"] = _mas(t_ys=np.array([TY0, 5, -1], np.int32))
    c["mas-t_y_Ty+1"] = _mas(t_ys=np.array([TY0, 5, TY0 + 1], np.int32))
    c["mas-t_x_-1"] = _mas(t_xs=np.array([TX0, 3, -1], np.int32))
    c["mas-t_x_Tx+1"] = _mas(t_xs=np.array([TX0, 3, TX0 + 1], np.int32))
    c["mas-Tx_above_the_LDS_bound"] = _mas(Tx=20481, B=1, t_xs=np.array([4], np.int32), t_ys=np.array([6], np.int32))

    for arg in ("x", "w", "y"):
        c[f"conv1d-null_{arg}"] = _conv(**{arg: None})
    c["conv1d-B_0"] = _conv(B=0)
    c["conv1d-T_0"] = _conv(T=0)
    c["conv1d-K_0"] = _conv(K=0)
    c["conv1d-dil_0"] = _conv(dil=0)
    c["conv1d-Cin_24"] = _conv(Cin=24)
    c["conv1d-halo"] = _conv(K=11, dil=7)
    c["conv1d-item_of_2_GiB"] = _conv(T=1 << 25)

    def probe(lib):
        ghz = (ctypes.c_double * 1)()
        return lib._fn("debug_clock_probe")(0, 1000, ghz, 0)
    c["clock_probe-n_0"] = probe
    return c


BAD_CALLS = _bad_calls()

EXPECTED = {
    'clock_probe-n_0': (-1, 'clock probe: bad arguments'),
    'conv1d-B_0': (1, 'bad argument'),
    'conv1d-Cin_24': (4, 'C_in must be a multiple of 16'),
    'conv1d-K_0': (1, 'bad argument'),
    'conv1d-T_0': (1, 'bad argument'),
    'conv1d-dil_0': (1, 'bad argument'),
    'conv1d-halo': (4, '(K-1)*dil > 64'),
    'conv1d-item_of_2_GiB': (1, "one item's tensor must stay below 2 GiB (32-bit offsets inside an item)"),
    'conv1d-null_w': (1, 'bad argument'),
    'conv1d-null_x': (1, 'bad argument'),
    'conv1d-null_y': (1, 'bad argument'),
    'mas-B_0': (1, 'bad argument'),
    'mas-Tx_0': (1, 'bad argument'),
    'mas-Tx_above_the_LDS_bound': (1, 'T_x 20481 too large for the LDS row buffers'),
    'mas-Ty_0': (1, 'bad argument'),
    'mas-null_paths': (1, 'bad argument'),
    'mas-null_t_xs': (1, 'bad argument'),
    'mas-null_t_ys': (1, 'bad argument'),
    'mas-null_values': (1, 'bad argument'),
    'mas-t_x_-1': (1, 'extent out of range'),
    'mas-t_x_Tx+1': (1, 'extent out of range'),
    'mas-t_y_-1': (1, 'extent out of range'),
    'mas-t_y_Ty+1': (1, 'extent out of range'),
    'mono_couple-B_0': (1, 'mono couple: bad arguments'),
    'mono_couple-B_65536': (1, 'mono couple: bad arguments'),
    'mono_couple-C_48': (4, 'mono couple: width 48 not built (a multiple of 32 in [32, 192])'),
    'mono_couple-T_0': (1, 'mono couple: bad arguments'),
    'mono_couple-len_-1': (1, 'mono couple: length -1 of item 2 outside [0, 40]'),
    'mono_couple-len_T+1': (1, 'mono couple: length 41 of item 2 outside [0, 40]'),
    'mono_couple-mode_2': (1, 'mono couple: bad arguments'),
    'mono_couple-null_W': (1, 'mono couple: bad arguments'),
    'mono_couple-null_b': (1, 'mono couple: bad arguments'),
    'mono_couple-null_h': (1, 'mono couple: bad arguments'),
    'mono_couple-null_lengths': (1, 'mono couple: bad arguments'),
    'mono_couple-null_u': (1, 'mono couple: bad arguments'),
    'mono_couple-null_z': (1, 'mono couple: bad arguments'),
    'op_denoise-B_0': (1, 'denoise: bad argument'),
    'op_denoise-B_65536': (1, 'denoise: bad argument'),
    'op_denoise-N_0': (1, 'denoise: bad argument'),
    'op_denoise-N_2^31': (1, 'denoise: bad argument'),
    'op_denoise-len_-1': (1, 'denoise: length -1 of item 2 is below filter_length / 2 + 1 = 33'),
    'op_denoise-len_N+1': (1, 'denoise: length 513 of item 2 exceeds N = 512'),
    'op_denoise-len_below_half_filter': (1, 'denoise: length 32 of item 2 is below filter_length / 2 + 1 = 33'),
    'op_denoise-null_bias': (1, 'denoise: bad argument'),
    'op_denoise-null_lengths': (1, 'denoise: bad argument'),
    'op_denoise-null_out': (1, 'denoise: bad argument'),
    'op_denoise-null_x': (1, 'denoise: bad argument'),
    'op_limit-B_0': (1, 'limit: bad argument'),
    'op_limit-B_65536': (1, 'limit: bad argument'),
    'op_limit-N_0': (1, 'limit: bad argument'),
    'op_limit-N_2^31': (1, 'limit: bad argument'),
    'op_limit-len_-1': (1, 'limit: length -1 of item 2 outside [0, 512]'),
    'op_limit-len_N+1': (1, 'limit: length 513 of item 2 outside [0, 512]'),
    'op_limit-null_lengths': (1, 'limit: bad argument'),
    'op_limit-null_out': (1, 'limit: null output'),
    'op_limit-null_x': (1, 'limit: bad argument'),
    'op_limit_gain-B_0': (1, 'limit: bad argument'),
    'op_limit_gain-B_65536': (1, 'limit: bad argument'),
    'op_limit_gain-N_0': (1, 'limit: bad argument'),
    'op_limit_gain-N_2^31': (1, 'limit: bad argument'),
    'op_limit_gain-len_-1': (1, 'limit: length -1 of item 2 outside [0, 512]'),
    'op_limit_gain-len_N+1': (1, 'limit: length 513 of item 2 outside [0, 512]'),
    'op_limit_gain-null_lengths': (1, 'limit: bad argument'),
    'op_limit_gain-null_out': (1, 'limit: null output'),
    'op_limit_gain-null_x': (1, 'limit: bad argument'),
    'op_loudness-B_0': (1, 'loudness: bad argument'),
    'op_loudness-B_65536': (1, 'loudness: bad argument'),
    'op_loudness-N_0': (1, 'loudness: bad argument'),
    'op_loudness-N_2^31': (1, 'loudness: bad argument'),
    'op_loudness-len_-1': (1, 'loudness: length -1 of item 2 outside [0, 512]'),
    'op_loudness-len_N+1': (1, 'loudness: length 513 of item 2 outside [0, 512]'),
    'op_loudness-null_lengths': (1, 'loudness: bad argument'),
    'op_loudness-null_x': (1, 'loudness: bad argument'),
    'op_loudness_limit-B_0': (1, 'limit: bad argument'),
    'op_loudness_limit-B_65536': (1, 'limit: bad argument'),
    'op_loudness_limit-N_0': (1, 'limit: bad argument'),
    'op_loudness_limit-N_2^31': (1, 'limit: bad argument'),
    'op_loudness_limit-len_-1': (1, 'limit: length -1 of item 2 outside [0, 512]'),
    'op_loudness_limit-len_N+1': (1, 'limit: length 513 of item 2 outside [0, 512]'),
    'op_loudness_limit-null_lengths': (1, 'limit: bad argument'),
    'op_loudness_limit-null_out': (1, 'limit: null output'),
    'op_loudness_limit-null_x': (1, 'limit: bad argument'),
    'op_loudness_normalize-B_0': (1, 'loudness: bad argument'),
    'op_loudness_normalize-B_65536': (1, 'loudness: bad argument'),
    'op_loudness_normalize-N_0': (1, 'loudness: bad argument'),
    'op_loudness_normalize-N_2^31': (1, 'loudness: bad argument'),
    'op_loudness_normalize-len_-1': (1, 'loudness: length -1 of item 2 outside [0, 512]'),
    'op_loudness_normalize-len_N+1': (1, 'loudness: length 513 of item 2 outside [0, 512]'),
    'op_loudness_normalize-null_lengths': (1, 'loudness: bad argument'),
    'op_loudness_normalize-null_out': (1, 'loudness: null output'),
    'op_loudness_normalize-null_x': (1, 'loudness: bad argument'),
    'op_pitch_formant_gain-B_0': (1, 'pitch: bad argument'),
    'op_pitch_formant_gain-B_65536': (1, 'pitch: bad argument'),
    'op_pitch_formant_gain-N_0': (1, 'pitch: bad argument'),
    'op_pitch_formant_gain-N_2^31': (1, 'pitch: bad argument'),
    'op_pitch_formant_gain-identity': (1, 'pitch: 0 semitones is the identity (P = Q): there is no gain to return'),
    'op_pitch_formant_gain-len_-1': (1, 'pitch: length -1 of item 2 outside [0, N = 512]'),
    'op_pitch_formant_gain-len_N+1': (1, 'pitch: length 513 of item 2 outside [0, N = 512]'),
    'op_pitch_formant_gain-null_lengths': (1, 'pitch: bad argument'),
    'op_pitch_formant_gain-null_out': (1, 'pitch: bad argument'),
    'op_pitch_formant_gain-null_x': (1, 'pitch: bad argument'),
    'op_pitch_shift-B_0': (1, 'pitch: bad argument'),
    'op_pitch_shift-B_65536': (1, 'pitch: bad argument'),
    'op_pitch_shift-N_0': (1, 'pitch: bad argument'),
    'op_pitch_shift-N_2^31': (1, 'pitch: bad argument'),
    'op_pitch_shift-len_-1': (1, 'pitch: length -1 of item 2 outside [0, N = 512]'),
    'op_pitch_shift-len_N+1': (1, 'pitch: length 513 of item 2 outside [0, N = 512]'),
    'op_pitch_shift-null_lengths': (1, 'pitch: bad argument'),
    'op_pitch_shift-null_out': (1, 'pitch: bad argument'),
    'op_pitch_shift-null_x': (1, 'pitch: bad argument'),
    'op_pitch_shift_formant-B_0': (1, 'pitch: bad argument'),
    'op_pitch_shift_formant-B_65536': (1, 'pitch: bad argument'),
    'op_pitch_shift_formant-N_0': (1, 'pitch: bad argument'),
    'op_pitch_shift_formant-N_2^31': (1, 'pitch: bad argument'),
    'op_pitch_shift_formant-len_-1': (1, 'pitch: length -1 of item 2 outside [0, N = 512]'),
    'op_pitch_shift_formant-len_N+1': (1, 'pitch: length 513 of item 2 outside [0, N = 512]'),
    'op_pitch_shift_formant-null_lengths': (1, 'pitch: bad argument'),
    'op_pitch_shift_formant-null_out': (1, 'pitch: bad argument'),
    'op_pitch_shift_formant-null_x': (1, 'pitch: bad argument'),
    'op_pitch_stretch-B_0': (1, 'pitch: bad argument'),
    'op_pitch_stretch-B_65536': (1, 'pitch: bad argument'),
    'op_pitch_stretch-N_0': (1, 'pitch: bad argument'),
    'op_pitch_stretch-N_2^31': (1, 'pitch: bad argument'),
    'op_pitch_stretch-identity': (1, 'pitch: 0 semitones is the identity (P = Q): there is no stretch to return'),
    'op_pitch_stretch-len_-1': (1, 'pitch: length -1 of item 2 outside [0, N = 512]'),
    'op_pitch_stretch-len_N+1': (1, 'pitch: length 513 of item 2 outside [0, N = 512]'),
    'op_pitch_stretch-null_lengths': (1, 'pitch: bad argument'),
    'op_pitch_stretch-null_out': (1, 'pitch: bad argument'),
    'op_pitch_stretch-null_x': (1, 'pitch: bad argument'),
    'op_pitch_stretch_formant-B_0': (1, 'pitch: bad argument'),
    'op_pitch_stretch_formant-B_65536': (1, 'pitch: bad argument'),
    'op_pitch_stretch_formant-N_0': (1, 'pitch: bad argument'),
    'op_pitch_stretch_formant-N_2^31': (1, 'pitch: bad argument'),
    'op_pitch_stretch_formant-identity': (1, 'pitch: 0 semitones is the identity (P = Q): there is no stretch to return'),
    'op_pitch_stretch_formant-len_-1': (1, 'pitch: length -1 of item 2 outside [0, N = 512]'),
    'op_pitch_stretch_formant-len_N+1': (1, 'pitch: length 513 of item 2 outside [0, N = 512]'),
    'op_pitch_stretch_formant-null_lengths': (1, 'pitch: bad argument'),
    'op_pitch_stretch_formant-null_out': (1, 'pitch: bad argument'),
    'op_pitch_stretch_formant-null_x': (1, 'pitch: bad argument'),
    'op_resample-B_0': (1, 'resample: bad argument'),
    'op_resample-B_65536': (1, 'resample: bad argument'),
    'op_resample-N_0': (1, 'resample: bad argument'),
    'op_resample-N_2^31': (1, 'resample: bad argument'),
    'op_resample-len_-1': (1, 'resample: length -1 of item 2 outside [0, 512]'),
    'op_resample-len_N+1': (1, 'resample: length 513 of item 2 outside [0, 512]'),
    'op_resample-null_lengths': (1, 'resample: bad argument'),
    'op_resample-null_out': (1, 'resample: bad argument'),
    'op_resample-null_x': (1, 'resample: bad argument'),
    'op_true_peak-B_0': (1, 'limit: bad argument'),
    'op_true_peak-B_65536': (1, 'limit: bad argument'),
    'op_true_peak-N_0': (1, 'limit: bad argument'),
    'op_true_peak-N_2^31': (1, 'limit: bad argument'),
    'op_true_peak-len_-1': (1, 'limit: length -1 of item 2 outside [0, 512]'),
    'op_true_peak-len_N+1': (1, 'limit: length 513 of item 2 outside [0, 512]'),
    'op_true_peak-null_lengths': (1, 'limit: bad argument'),
    'op_true_peak-null_out': (1, 'limit: null output'),
    'op_true_peak-null_x': (1, 'limit: bad argument'),
    'plain_attention-B_0': (1, 'plain attention: bad arguments'),
    'plain_attention-B_65536': (1, 'plain attention: bad arguments'),
    'plain_attention-C_not_a_multiple_of_heads': (1, 'plain attention: bad arguments'),
    'plain_attention-T_0': (1, 'plain attention: bad arguments'),
    'plain_attention-head_dim_40': (4, 'plain attention: head dim 40 not built'),
    'plain_attention-len_-1': (1, 'plain attention: length -1 of item 2 outside [0, 40]'),
    'plain_attention-len_T+1': (1, 'plain attention: length 41 of item 2 outside [0, 40]'),
    'plain_attention-null_lengths': (1, 'plain attention: bad arguments'),
    'plain_attention-null_out': (1, 'plain attention: bad arguments'),
    'plain_attention-null_qkv': (1, 'plain attention: bad arguments'),
    'relpos_attention-B_0': (1, 'relpos attention: bad arguments'),
    'relpos_attention-B_65536': (1, 'relpos attention: bad arguments'),
    'relpos_attention-C_not_a_multiple_of_heads': (1, 'relpos attention: bad arguments'),
    'relpos_attention-T_0': (1, 'relpos attention: bad arguments'),
    'relpos_attention-ek_only': (1, 'relpos attention: bad arguments'),
    'relpos_attention-ev_only': (1, 'relpos attention: bad arguments'),
    'relpos_attention-head_dim_16': (4, 'relpos attention: head dim 16 not built'),
    'relpos_attention-len_-1': (1, 'relpos attention: length -1 of item 2 outside [0, 40]'),
    'relpos_attention-len_T+1': (1, 'relpos attention: length 41 of item 2 outside [0, 40]'),
    'relpos_attention-null_lengths': (1, 'relpos attention: bad arguments'),
    'relpos_attention-null_out': (1, 'relpos attention: bad arguments'),
    'relpos_attention-null_qkv': (1, 'relpos attention: bad arguments'),
    'relpos_attention-window_5': (4, 'relpos attention: window 5 not in [0, 4]'),
}


def test_the_table_and_the_record_name_the_same_calls():
    assert sorted(BAD_CALLS) == sorted(EXPECTED)


@pytest.mark.parametrize("case", sorted(BAD_CALLS))
def test_refused_before_the_first_hip_call(hip_lib, case):
    rc = BAD_CALLS[case](hip_lib)
    assert (rc, hip_lib._fn("last_error")().decode()) == EXPECTED[case]


def _ragged(seed):
    """x with NaN at and beyond each length, y full of NaN, in heap arrays of exactly [B, N]"""
    x = np.random.default_rng(seed).standard_normal((B0, N0)).astype(np.float32)
    ln = np.array([0, 100, N0], np.int64)
    for b, n in enumerate(ln):
        x[b, n:] = np.nan
    return x, ln, np.full((B0, N0), np.nan, np.float32)


@pytest.mark.parametrize("door, scalars", [("op_resample", (16000, 16000)), ("op_pitch_shift", (0.0,)), ("op_pitch_shift_formant", (0.0,))])
def test_identity_paths_are_host_only(hip_lib, door, scalars):
    """rate_in == rate_out and P == Q: the input with zeros at and beyond each length, and no device is touched (there is none here)"""
    x, ln, y = _ragged(7)
    assert hip_lib._fn(door)(0, _ptr(x), _ptr(ln, I64), B0, N0, *scalars, _ptr(y)) == 0
    for b, n in enumerate(ln):
        assert np.array_equal(y[b, :n], x[b, :n]) and not y[b, n:].any()


def test_clock_probe_error_raises(hip_lib):
    with pytest.raises(VitsError, match="clock probe: bad arguments") as e:
        hip_lib.clock_probe(n=0)
    assert e.value.code == 1
