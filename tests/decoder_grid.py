"""The table of decoder geometries tests/test_decoder_geometry.py (CPU) and tests/test_decoder_geometry_gpu.py (GPU) walk: data only.

Every row follows the loader's rules (engine_model.hip.h load_decoder, mirrored by weights.validate_hparams), so vits_create has to
accept it: rate u <= 8, kernel Ku a multiple of u with Ku - u even, C % 64 == 0 at every stage input, 1-3 ResBlock chains of odd
kernels, 1-4 dilations with (K - 1) * d <= 64, n_fft % hop == 0, a tail that fits 64 KiB of LDS.  Not a cross product: every value of
every axis occurs at least twice, with different partners (test_grid_counts_and_axes).

Row: (name, dec_type, ups ((u, Ku), ...), res_kernels, res_dilations (one list, or one per chain), tail, dec_initial_channel,
inter_channels, voice).  tail: (subbands, n_fft, hop, taps) for dec_type 0 / 2, (n_fft, hop) for 3, None for 1.  voice = True: a full
tiny voice around the decoder (speaker conditioning: the plain Generator's cond(g)); False: a vocoder-only blob.

What the reference's own modules can build of this (tools/gen_golden_decoder_geometry.py): ResBlock1 has exactly 3 dilations, PQMF() is
always 4 bands / 62 taps, the multi-stream synthesis filter always 63 taps.  Rows outside that (n_resd != 3, other S / taps) rest on the
float64 restatement (tests/decoder_ref.py) alone -- and, for dec_type 0 / 1, on the C oracle, which is general over all of them.
"""
import functools

K1, K2A, K2B, K3A, K3B = (3,), (3, 7), (5, 11), (3, 5, 7), (3, 7, 11)
D1, D2A, D2B, D2C, D3, D4 = (1,), (1, 2), (2, 6), (3, 12), (1, 3, 5), (1, 3, 5, 9)
D4K11 = (1, 2, 4, 6)  # 4 dilations under kernel 11: (11 - 1) * 6 = 60 <= 64

GRID = [
    # ---- dec_type 0: multi-band iSTFT (PQMF synthesis)
    ("mb_default", 0, ((4, 16), (4, 16)), K3B, D3, (4, 16, 4, 62), 512, 64, False),
    ("mb_u3_nooverlap", 0, ((3, 3),), K1, D1, (4, 16, 16, 62), 64, 64, False),
    ("mb_u5_u2", 0, ((5, 5), (2, 2)), K2A, D3, (4, 16, 8, 62), 128, 64, False),
    ("mb_2x8_3x9", 0, ((2, 8), (3, 9)), K2B, ((1, 3, 5), (2, 6, 1)), (4, 8, 2, 62), 256, 64, False),
    ("mb_u7_d4", 0, ((7, 7),), K3A, D4, (4, 32, 8, 62), 128, 64, False),
    ("mb_u1_3stage_d4", 0, ((1, 3), (2, 4), (2, 2)), K2A, D4, (4, 32, 4, 62), 256, 64, False),
    ("mb_u6_u4_s2", 0, ((6, 6), (4, 4)), K1, D2C, (2, 8, 2, 30), 128, 64, False),
    ("mb_u8_s8", 0, ((8, 8), (2, 4)), K3A, D3, (8, 32, 8, 126), 256, 64, False),
    ("mb_4x12_5x15_k11d4", 0, ((4, 12), (5, 15)), K2B, (D4, D4K11), (4, 16, 4, 30), 128, 64, False),
    ("mb_6x18_8x24", 0, ((6, 18), (8, 24)), K1, D2A, (4, 16, 4, 126), 128, 64, False),
    ("mb_8x16_3x9_s1", 0, ((8, 16), (3, 9)), K3B, (D4, D4, D4K11), (1, 16, 4, 62), 512, 64, False),
    ("mb_4stage", 0, ((2, 2), (2, 4), (3, 3), (1, 3)), K2A, (D2C, D2A), (4, 16, 4, 62), 512, 64, False),
    # ---- dec_type 2: multi-stream iSTFT (learned synthesis filter, biased post conv)
    ("ms_u4_nooverlap", 2, ((4, 4), (4, 16)), K3A, D3, (4, 16, 16, 62), 128, 64, False),
    ("ms_5x15", 2, ((5, 15),), K2B, D2B, (4, 16, 8, 62), 64, 64, False),
    ("ms_u7_2x8", 2, ((7, 7), (2, 8)), K1, D1, (4, 8, 2, 62), 256, 64, False),
    ("ms_8x24", 2, ((8, 24),), K2A, D2A, (4, 32, 8, 62), 128, 64, False),
    ("ms_u6_u5", 2, ((6, 6), (5, 5)), K3B, D3, (4, 32, 4, 62), 512, 64, False),
    ("ms_3stage_s2", 2, ((3, 9), (2, 2), (2, 4)), K1, D2C, (2, 8, 2, 30), 256, 64, False),
    ("ms_4x12_u1_s8", 2, ((4, 12), (1, 3)), K2A, D4, (8, 32, 8, 126), 128, 64, False),
    ("ms_u8_taps30", 2, ((8, 8),), K3A, D1, (4, 16, 4, 30), 64, 64, False),
    ("ms_2x4_6x18_taps126", 2, ((2, 4), (6, 18)), K2B, (D2B, D2A), (4, 16, 4, 126), 256, 64, False),
    ("ms_8x16_s1", 2, ((8, 16), (2, 2)), K1, D4, (1, 16, 4, 62), 128, 64, False),
    ("ms_4stage", 2, ((2, 8), (2, 4), (2, 2), (2, 2)), K3B, D3, (4, 16, 4, 62), 512, 64, False),
    # ---- dec_type 3: single-band iSTFT
    ("is_default", 3, ((8, 16), (8, 16)), K3B, D3, (16, 4), 512, 64, False),
    ("is_u4_nooverlap", 3, ((4, 4),), K1, D2B, (16, 16), 128, 64, False),
    ("is_u3_5x15", 3, ((3, 3), (5, 15)), K2A, D1, (8, 2), 256, 64, False),
    ("is_u7_3x9", 3, ((7, 7), (3, 9)), K3A, D2A, (32, 8), 128, 64, False),
    ("is_6x18_n64", 3, ((6, 18),), K2B, D2A, (64, 16), 64, 64, False),
    ("is_u1_4x12_n64h4", 3, ((1, 3), (4, 12)), K1, D4, (64, 4), 256, 64, False),
    ("is_u5_u6", 3, ((5, 5), (6, 6)), K2B, D2B, (16, 4), 512, 64, False),
    ("is_3stage_d4", 3, ((2, 2), (8, 24), (2, 8)), K3A, D4, (16, 16), 256, 64, False),
    ("is_4x16_u7_perchain", 3, ((4, 16), (7, 7)), K2A, ((1, 3, 5), (2, 6, 1)), (8, 2), 128, 64, False),
    ("is_u8_u4", 3, ((8, 8), (4, 4)), K3B, D1, (32, 8), 256, 64, False),
    ("is_2x4_n64", 3, ((2, 4),), K3A, D3, (64, 16), 128, 64, False),
    ("is_4stage", 3, ((3, 3), (2, 2), (2, 2), (2, 2)), K1, D3, (64, 4), 512, 64, False),
    # ---- dec_type 1: the plain HiFi-GAN Generator (tanh tail); cond(g) only exists in a full voice
    ("hg_v1", 1, ((8, 16), (8, 16), (2, 4), (2, 4)), K3B, D3, None, 512, 80, False),
    ("hg_u5_u4", 1, ((5, 5), (4, 4)), K2A, D2A, None, 128, 80, False),
    ("hg_u6_d4", 1, ((6, 6),), K1, D4, None, 64, 64, False),
    ("hg_3stage", 1, ((7, 7), (8, 8), (1, 3)), K2B, D2B, None, 256, 64, False),
    ("hg_cond_4x12_u3", 1, ((4, 12), (3, 3)), K3A, D3, None, 128, 64, True),
    ("hg_cond_2x8_6x18", 1, ((2, 8), (6, 18)), K1, D1, None, 256, 64, True),
    ("hg_5x15_8x24", 1, ((5, 15), (8, 24)), K3A, D1, None, 512, 80, False),
    ("hg_4x16", 1, ((4, 16),), K2B, D3, None, 128, 80, False),
]

# Geometries the loader must refuse: (name, row fields as above, hparams field overrides applied after decoder_hparams, expected error
# code name, a regex both the library's message and validate_hparams' ValueError must match -- it names the offending value)
REFUSED = [
    ("kernel_not_multiple", (0, ((5, 11),), K1, D1, (4, 16, 4, 62), 64, 64), {}, "UNSUPPORTED", r"rate 5 / kernel 11"),
    ("kernel_minus_rate_odd", (0, ((5, 10),), K1, D1, (4, 16, 4, 62), 64, 64), {}, "UNSUPPORTED", r"rate 5 / kernel 10"),
    ("rate_9", (1, ((9, 9),), K1, D1, None, 64, 64), {}, "UNSUPPORTED", r"rate 9 / kernel 9"),
    ("channels_32_at_stage_2", (3, ((2, 4), (2, 4), (2, 4)), K1, D1, (16, 4), 128, 64), {}, "UNSUPPORTED", r"stage 2: 32 input channels"),
    ("four_chains", (0, ((4, 16),), (3, 5, 7, 9), D1, (4, 16, 4, 62), 64, 64), {}, "UNSUPPORTED", r"n_resk 4"),
    ("halo_66", (2, ((4, 16),), K1, (1, 33), (4, 16, 4, 62), 64, 64), {}, "UNSUPPORTED", r"kernel 3 with dilation 33: a halo of 66"),
    ("even_resblock_kernel", (1, ((4, 16),), (4,), D1, None, 64, 64), {}, "BLOB", r"resblock kernel 4 invalid"),
    ("tail_lds", (3, ((4, 16),), K1, D1, (128, 32), 64, 64), {}, "UNSUPPORTED", r"n_fft 128, hop 32.*LDS"),
    ("hop_length", (0, ((4, 16),), K1, D1, (4, 16, 4, 62), 64, 64), {"hop_length": 65}, "BLOB", r"64 samples per frame but hop_length is 65"),
]

N_GRID, N_REFUSED = 43, 9

AXES = {
    "res_kernels": [K1, K2A, K2B, K3A, K3B],
    "res_dilations": [D1, D2A, D2B, D2C, D3, D4, D4K11],
    "ups": [(1, 3), (2, 2), (2, 4), (2, 8), (3, 3), (3, 9), (4, 4), (4, 12), (4, 16), (5, 5), (5, 15), (6, 6), (6, 18), (7, 7), (8, 8),
            (8, 16), (8, 24)],
    "stages_from": [(1, 64), (1, 128), (2, 128), (2, 256), (2, 512), (3, 256), (4, 512)],
    "tail_mb": [(4, 16, 4, 62), (4, 16, 16, 62), (4, 16, 8, 62), (4, 8, 2, 62), (4, 32, 8, 62), (4, 32, 4, 62), (2, 8, 2, 30), (8, 32, 8, 126),
                (4, 16, 4, 30), (4, 16, 4, 126), (1, 16, 4, 62)],
    "tail_istft": [(16, 4), (16, 16), (8, 2), (32, 8), (64, 16), (64, 4)],
    "plain": [(False, 80), (False, 64), (True, 64)],  # (cond(g), inter_channels)
}


def chains(row):
    """the per-chain dilation lists of a row"""
    rk, rd = row[3], row[4]
    return list(rd) if isinstance(rd[0], tuple) else [rd] * len(rk)


def axis_values(row):
    """{axis: set of the axis values this row carries}"""
    _, dt, ups, rk, _, tail, C0, I, voice = row
    out = {"res_kernels": {rk}, "res_dilations": set(chains(row)), "ups": set(ups), "stages_from": {(len(ups), C0)}}
    if dt in (0, 2):
        out["tail_mb"] = {tail}
    elif dt == 3:
        out["tail_istft"] = {tail}
    else:
        out["plain"] = {(voice, I)}
    return out


def row_hparams(row, conv_precision=0, voice=None):
    """voice: None = as the row says; True = the tiny voice around the row's decoder (ragged / fast-path legs)"""
    from vosk_tts_amd import weights as W

    _, dt, ups, rk, rd, tail, C0, I, row_voice = row
    voice = row_voice if voice is None else voice
    return W.decoder_hparams(dt, ups, rk, rd, tail, C0, I, n_vocab=20 if voice else 0, conv_precision=conv_precision)


def refused_hparams(entry):
    from vosk_tts_amd import weights as W

    _, (dt, ups, rk, rd, tail, C0, I), over, _, _ = entry
    hp = W.decoder_hparams(dt, ups, rk, rd, tail, C0, I)
    for k, v in over.items():
        setattr(hp, k, v)
    return hp


def row_id(row):
    return row[0]


@functools.lru_cache(maxsize=None)
def row_weights(name, seed=1234):
    """(hparams, synthetic tensors) of the row called `name`"""
    from vosk_tts_amd import weights as W

    hp = row_hparams({r[0]: r for r in GRID}[name])
    return hp, W.make_synthetic_weights(hp, seed)


@functools.lru_cache(maxsize=None)
def measured_field(name):
    """(left, right) reach of row `name` in latent frames (decoder_ref.receptive_field on a probe long enough to hold it)"""
    from decoder_ref import receptive_field

    hp, tens = row_weights(name)
    T = 65
    while True:
        try:
            return receptive_field(hp, tens, T_y=T)
        except AssertionError:
            T = 2 * T - 1
            if T > 600:
                raise
