// dec_end_rules.h -- the launch rules of the single utterance's decoder end as pure host arithmetic, and the two environment switches
// they read: which K-split launches split by chunk (ks_chunk_rule), which of those give a workgroup two column tiles (ks_pair_rule),
// which fused tails run the compile-time geometry's body (tail_fixed_rule).  No HIP, no engine types: the engine calls these
// (ks_chunk_takes / ks_pair_takes in engine_launch.hip.h, tail_fixed_geometry in engine_stages.hip.h) and tests/test_dec_end_rules.py
// compiles them into a host program and asserts them on the four K-split launches of the c2 shape.
#pragma once
#include <cstdlib>

#define KS_SLAB_PITCH 64  // floats per column tile of a wave's slab (ks_chunk_body, conv_mfma.hip.h)

// VITS_KS_PAIR: column-pair workgroups of the chunk split: 0 = never, 1 = ks_pair_rule (default), 2 = wherever there are two column tiles (tests)
inline int ks_pair_mode_env() {
  const char* v = getenv("VITS_KS_PAIR");
  return v ? atoi(v) : 1;
}
// VITS_TAIL_GENERIC=1: the run-time tail body for every geometry
inline bool tail_generic_env() {
  const char* v = getenv("VITS_TAIL_GENERIC");
  return v && atoi(v) != 0;
}

// the shape part of ks_chunk_takes (the caller has checked the instantiation: 16 waves, one 32 x 32 STORE tile, one group): at least 4
// taps to share a window of at most KS_SLAB_PITCH columns, rows long enough for the vector loads, a grid of about one workgroup per CU
inline bool ks_chunk_rule(int K, int dil, int Tin, long nblk, long n_cu) {
  if (K < 4 || dil < 1 || 32 + (K - 1) * dil > KS_SLAB_PITCH || Tin < 4) return false;
  return 4 * nblk <= 5 * n_cu;
}
// a chunk-split launch in column pairs: 4 taps (the pair form's only tap count), 64 + halo inside the pair's slab pitch, no compact tile
// map (it counts single tiles), at least two column tiles; mode 1: more than one round of the chip in single tiles, at most one in pairs
inline bool ks_pair_rule(int mode, int K, int dil, int ntiles_m, int ntiles_n, int B, bool tile_map, long nblk, long n_cu) {
  if (!mode || tile_map || ntiles_n < 2 || K != 4 || 64 + (K - 1) * dil > 2 * KS_SLAB_PITCH) return false;
  if (mode == 2) return true;
  return nblk > n_cu && (long)ntiles_m * ((ntiles_n + 1) / 2) * B <= n_cu;
}
// the fused tail's compile-time geometries: (4, 16, 4, 62) and the single-band N 16 / hop 4
inline bool tail_fixed_rule(bool generic, bool synth, int S, int N, int hop, int taps) {
  return !generic && N == 16 && hop == 4 && (!synth || (S == 4 && taps == 62));
}
