"""The launch rules of the single utterance's decoder end (csrc/dec_end_rules.h: ks_chunk_rule, ks_pair_rule, tail_fixed_rule and the
switches VITS_KS_PAIR / VITS_TAIL_GENERIC they read), compiled into a host program with the C++ compiler and asserted -- no GPU.

The engine's ks_chunk_takes / ks_pair_takes (csrc/engine_launch.hip.h) and tail_fixed_geometry (csrc/engine_stages.hip.h) are calls of
these functions with the launch's own numbers, and ConvSelect reads VITS_KS_PAIR through ks_pair_mode_env, so what is asserted here is
what decides the grids.  (A launch's grid is not visible from Python and the ABI test pins the debug hooks; tests/test_dec_end_gpu.py
runs this program under each child's environment, so that its identity tests cannot pass with the switch unread.)

  * the four K-split launches of the c2 decoder shape (B = 1, 150 frames, 256 CUs): conv_pre 192 -> 512, 7 taps, T 150: 16 x 5 = 80
    workgroups; ups[0] 512 -> 4 phases x 256 rows, 4 taps, T 150: 32 x 5 = 160; ups[1] 256 -> 4 x 128 rows, 4 taps, T 600: 16 x 19 =
    304; conv_post 128 -> 72 rows (96 padded), 7 taps, T + 1 = 2401 columns: 3 x 76 = 228.  Default switch: all four split by chunk,
    ups[1] alone goes in pairs, 16 x 10 = 160 workgroups; the other three keep their grids.  VITS_KS_PAIR=0: none.  2: ups[0] and
    ups[1] (4 taps), never the 7-tap launches;
  * the gates one by one: a compact tile map, a single column tile, 7 taps, a window beyond the pitch, a single-tile grid of at most
    one round, rows shorter than a vector load, a grid beyond 5/4 rounds (no chunk split, so no pairs; at 256 CUs a chunk-split grid
    of at most 320 single tiles is never more than 213 pairs, so the "at most one round in pairs" gate cannot be the one that decides);
  * the tail: (4, 16, 4, 62) and single-band (16, 4) take the compile-time body, every neighbouring geometry does not, and
    VITS_TAIL_GENERIC=1 turns it off for all.
"""
import json
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "vosk_tts_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include "dec_end_rules.h"
struct L { const char* name; int K, dil, Tin, m, n, B; bool map; };
int main() {
  const int mode = ks_pair_mode_env();
  const long cus = 256;
  const L ls[] = {
      {"conv_pre", 7, 1, 150, 16, 5, 1, false},   {"ups0", 4, 1, 150, 32, 5, 1, false},
      {"ups1", 4, 1, 600, 16, 19, 1, false},      {"conv_post", 7, 1, 2400, 3, 76, 1, false},
      {"ups1_tile_map", 4, 1, 600, 16, 19, 1, true}, {"ups1_one_tile", 4, 1, 32, 300, 1, 1, false},
      {"ups1_dil_22", 4, 22, 600, 16, 19, 1, false}, {"ups1_17_rows", 4, 1, 600, 17, 19, 1, false},
      {"ups1_short", 4, 1, 480, 16, 15, 1, false}, {"ups1_b2", 4, 1, 600, 16, 19, 2, false},
      {"ups1_t3", 4, 1, 3, 16, 19, 1, false},      {"conv_t64", 4, 1, 64, 2, 2, 1, false},
      {"conv_t64_k7", 7, 1, 64, 2, 2, 1, false},   {"conv_t33_b2", 4, 1, 33, 1, 2, 2, false},
  };
  printf("{\"mode\": %d, \"launches\": {", mode);
  for (unsigned i = 0; i < sizeof ls / sizeof ls[0]; ++i) {
    const L& l = ls[i];
    const long nblk = (long)l.m * l.n * l.B;
    const bool chunk = ks_chunk_rule(l.K, l.dil, l.Tin, nblk, cus);
    const bool pair = chunk && ks_pair_rule(mode, l.K, l.dil, l.m, l.n, l.B, l.map, nblk, cus);
    printf("%s\"%s\": [%d, %d, %ld]", i ? ", " : "", l.name, chunk ? 1 : 0, pair ? 1 : 0, pair ? (long)l.m * ((l.n + 1) / 2) * l.B : nblk);
  }
  const bool g = tail_generic_env();
  struct T { const char* name; bool synth; int S, N, hop, taps; };
  const T ts[] = {{"mb_4_16_4_62", true, 4, 16, 4, 62}, {"mb_4_16_4_30", true, 4, 16, 4, 30}, {"mb_4_16_4_126", true, 4, 16, 4, 126},
                  {"mb_4_16_8_62", true, 4, 16, 8, 62}, {"mb_4_32_4_62", true, 4, 32, 4, 62}, {"mb_1_16_4_62", true, 1, 16, 4, 62},
                  {"mb_2_8_2_30", true, 2, 8, 2, 30},   {"is_16_4", false, 1, 16, 4, 0},       {"is_16_16", false, 1, 16, 16, 0},
                  {"is_64_4", false, 1, 64, 4, 0},      {"is_8_2", false, 1, 8, 2, 0}};
  printf("}, \"generic\": %d, \"tails\": {", g ? 1 : 0);
  for (unsigned i = 0; i < sizeof ts / sizeof ts[0]; ++i)
    printf("%s\"%s\": %d", i ? ", " : "", ts[i].name, tail_fixed_rule(g, ts[i].synth, ts[i].S, ts[i].N, ts[i].hop, ts[i].taps) ? 1 : 0);
  printf("}}\n");
  return 0;
}
"""


def build_rules_program(directory):
    """compiles PROGRAM against csrc/dec_end_rules.h into `directory` -> path of the executable"""
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "no C++ compiler found (the oracle's build needs one too)"
    src, exe = os.path.join(str(directory), "dec_end_rules_host.cpp"), os.path.join(str(directory), "dec_end_rules_host")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", exe, src], check=True, capture_output=True, text=True)
    return exe


def run_rules_program(exe, **env):
    """the program's answers under the environment `env` (VITS_KS_PAIR / VITS_TAIL_GENERIC removed unless given)"""
    e = {k: v for k, v in os.environ.items() if k not in ("VITS_KS_PAIR", "VITS_TAIL_GENERIC")}
    e.update(env)
    return json.loads(subprocess.run([exe], env=e, check=True, capture_output=True, text=True).stdout)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_rules_program(tmp_path_factory.mktemp("dec_end_rules"))


C2 = {"conv_pre": 80, "ups0": 160, "ups1": 304, "conv_post": 228}


def test_default_rule_pairs_ups1_of_c2_and_nothing_else(exe):
    r = run_rules_program(exe)
    assert r["mode"] == 1
    L = r["launches"]
    for name, grid in C2.items():
        chunk, pair, got = L[name]
        assert chunk == 1, f"{name}: the chunk split"
        assert (pair, got) == ((1, 160) if name == "ups1" else (0, grid)), f"{name}: pair {pair}, {got} workgroups"


def test_default_rule_gates(exe):
    L = run_rules_program(exe)["launches"]
    assert L["ups1_tile_map"] == [1, 0, 304]     # the compact tile map counts single tiles
    assert L["ups1_one_tile"] == [1, 0, 300]     # one column tile: nothing to pair
    assert L["ups1_dil_22"][1] == 0              # 64 + 66 columns do not fit the pair's pitch (nor 32 + 66 the single tile's)
    assert L["ups1_17_rows"] == [0, 0, 323]      # 323 > 5/4 of 256: the tap split, so no pairs (17 x 10 pairs would fit)
    assert L["ups1_short"] == [1, 0, 240]        # 240 workgroups are one round already
    assert L["ups1_b2"] == [0, 0, 608]           # two rounds and more: the tap split, no pairs
    assert L["ups1_t3"][0] == 0                  # rows shorter than a vector load
    assert L["conv_t64"] == [1, 0, 4] and L["conv_t64_k7"] == [1, 0, 4] and L["conv_t33_b2"] == [1, 0, 4]


@pytest.mark.parametrize("mode", ["0", "2"])
def test_switch_values(exe, mode):
    r = run_rules_program(exe, VITS_KS_PAIR=mode)
    assert r["mode"] == int(mode)
    L = r["launches"]
    if mode == "0":
        assert all(v[1] == 0 for v in L.values())
        assert [L[n][2] for n in C2] == list(C2.values())
    else:
        assert L["ups0"] == [1, 1, 96] and L["ups1"] == [1, 1, 160]          # 4 taps, two or more column tiles
        assert L["conv_pre"] == [1, 0, 80] and L["conv_post"] == [1, 0, 228]  # 7 taps: single tiles under every setting
        assert L["conv_t64"] == [1, 1, 2] and L["conv_t33_b2"] == [1, 1, 2] and L["conv_t64_k7"] == [1, 0, 4]
        assert L["ups1_tile_map"][1] == 0 and L["ups1_one_tile"][1] == 0 and L["ups1_b2"][1] == 0 and L["ups1_t3"][1] == 0


def test_tail_geometries(exe):
    r = run_rules_program(exe)
    assert r["generic"] == 0
    assert {k for k, v in r["tails"].items() if v} == {"mb_4_16_4_62", "is_16_4"}
    r = run_rules_program(exe, VITS_TAIL_GENERIC="1")
    assert r["generic"] == 1 and not any(r["tails"].values())
    assert run_rules_program(exe, VITS_TAIL_GENERIC="0")["tails"]["mb_4_16_4_62"] == 1
