/*
 * vits_watermark_payload.h — 16 payload bits inside the keyed audio watermark of include/vits_watermark.h, and a device reader that
 * returns them.  One service key marks everything; the tenant, the request or the day rides inside the mark, and one read returns it.
 *
 * An extension of the product library: the reference has no counterpart, so these entry points are checked against a float64
 * restatement of the definition below (tests/watermark_payload_ref.py, the authority, on top of tests/watermark_ref.py).  Same status
 * codes and vits_last_error as include/vits_mi355.h; all are re-entrant.  The key is the SELECTOR it is in vits_watermark.h, and the
 * payload is as public as the chips: anyone who knows the key reads it.
 *
 * Payload.  p in [0, 65535]; anything larger is VITS_ERR_ARG naming the value.
 *
 * Coded word.  W = (p << 8) | crc8(p), 24 bits.  crc8 runs over the 16 payload bits MSB first: polynomial 0x07, initial value 0xFF, no
 * final xor.  W(0) = 0x0000D7, W(0xBEEF) = 0xBEEFCD, crc8(0xFFFF) = 0xF3.  Coded bit i (0 .. 23) is (W >> (23 - i)) & 1.  The code has
 * minimum distance 4 (the lowest weight of the linear part, initial value 0, over all 65535 non-zero payloads is 4: checked
 * exhaustively by tests/test_watermark_payload.py), so up to three wrong bits never read as another payload.  The all-zero word is not
 * a codeword, because the initial value is 0xFF: that is why a plain mark does not read as "payload 0".
 *
 * Positions.  Geometry, band, tiles and mix are those of vits_watermark.h.  With mk = mix(key), position (q, j), q in [0, 16),
 * j in [0, 96), is a PILOT if (q + j) is odd, otherwise a PAYLOAD POSITION carrying coded bit
 *   i(q, j) = mix(mk ^ (0x80000000 | (96 q + j + 1))) mod 24.
 * 96 q + j + 1 is at most 1536, so these hash inputs never collide with the chips' own.
 *   c'(q, j) = c(key, q, j) on pilots, c(key, q, j) (1 - 2 bit_i(q, j)) on payload positions.
 * Integer arithmetic only: the device and the restatement agree bit for bit.  (For key 0x5EED1234 there are 752 scored pilot chips,
 * j in 1 .. 94, and the 24 bits get 23 to 41 scored chips each.)
 *
 * Embed.  Exactly the embed of vits_watermark.h with c' in place of c: same frames, same gains fp32(1 +- a), same overlap-add, same
 * rule for items below n/2 + 1 samples, exactly 0 at and beyond len.  depth_dB: 0 < depth_dB <= VITS_WATERMARK_MAX_DEPTH_DB;
 * 0 = VITS_WATERMARK_PAYLOAD_DEFAULT_DEPTH_DB = 2 dB.  The deeper default is what the bits need: each coded bit is read from about 30
 * chips where the detector has 1504, and at 1 dB one bit of 24 was wrong on 3 s of the test signal ("Watermark payload").
 * Like the 1 dB default of the plain mark it is a design choice, and nobody has run a listening test on it.
 *
 * Read.  Steps 1 to 5 of Detect (vits_watermark.h) unchanged: Lb, then G[q, j] per offset index o.  Then
 *   6'. zp_o = sum_{pilot, 1 <= j <= 94} c G / sqrt(sum_{pilot, 1 <= j <= 94} G^2); 0 without a complete row or with a zero denominator
 *   7'. o* = argmax_o zp_o, the lowest o on a tie; z = zp_{o*}; offset = 128 o*; rows as in Detect; detected iff
 *       z >= VITS_WATERMARK_THRESHOLD
 *   8'. at o*, for each coded bit i, over the payload positions with i(q, j) = i and 1 <= j <= 94:
 *       s_i = sum c G, n_i = sum G^2, z_i = s_i / sqrt(n_i) (0 where n_i = 0); bit_i = 1 iff z_i < 0
 *   9'. the bits packed into W'; payload = W' >> 8 is always reported; valid iff detected and crc8(W' >> 8) == (W' & 0xFF).
 * The Hoeffding argument of vits_watermark.h holds unchanged for step 7': for a key independent of the audio the pilot chips are
 * independent fair signs and zp_o is their sum under weights whose squares sum to 1, so P(zp_o >= t) <= exp(-t^2 / 2) and, over the 128
 * offsets at t = 6, the false-alarm bound stays 128 e^(-18) = 1.9e-6 per item.  `valid` asks for the CRC on top of that.
 *
 * Arithmetic.  As in Detect: the transforms, ln and Lb are fp32; T, D, G, every sum of steps 6' to 8' and the divisions are double.
 * Each sum runs in ascending 96 q + j, in a fixed order and without atomics: the same call twice gives the same bits, and an item does
 * not depend on its batch.
 *
 * Consequences.  A plain mark read with the same key is `detected` -- on half the chips, so at a lower z than
 * vits_op_watermark_detect gives -- and its word is 0x000000, which is not a codeword: valid = 0.  A payload mark is NOT a plain mark:
 * the chips of its payload positions are flipped wherever the coded bit is 1, so what vits_op_watermark_detect makes of it goes with
 * the weight of the word -- on 4 s of the test signal at 2 dB the restatement's detector scored 1.3 for payload 0xFFFF, 4.8 for 0xBEEF,
 * 8.4 for 0xA5A5 and 16.6 for 0x0000, whose word 0x0000D7 flips few chips -- and it is not a detector of payload marks.  A service that
 * uses payloads detects with the reader.  There is no error correction: one wrong bit makes
 * the read invalid, and bit_z shows which one was weak.  Robustness beyond crop, gain and int16 rounding is not claimed.
 */
#ifndef VITS_WATERMARK_PAYLOAD_H
#define VITS_WATERMARK_PAYLOAD_H

#include "vits_watermark.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VITS_WATERMARK_PAYLOAD_BITS 16
#define VITS_WATERMARK_CODED_BITS 24
#define VITS_WATERMARK_PAYLOAD_MAX 65535u
#define VITS_WATERMARK_PAYLOAD_DEFAULT_DEPTH_DB 2.0f

/* vits_synth_opts.flags / stts_synth_opts.flags: the mark of VITS_FLAG_WATERMARK carries a payload.  Honoured only together with
 * *_FLAG_WATERMARK; alone the call fails with VITS_ERR_ARG naming both.  The older structs keep their layouts; a caller that sets the
 * flag passes the extended struct below through the same pointer, and the two fields are read only when the flag is set.
 * watermark_payloads: NULL, or one value per item of a batch call ([B]); where it is not NULL it overrides the scalar.  A document is
 * marked as the one item it has become and takes the scalar.  watermark_depth_db = 0 then means 2 dB.  Honoured by the one-shot, batch,
 * marks and document entry points of both families; streams refuse the flag by name, as they refuse the plain mark.  The words are an
 * argument of each call, uploaded with it: nothing of a payload is kept between calls. */
#define VITS_FLAG_WATERMARK_PAYLOAD 512
#define STTS_FLAG_WATERMARK_PAYLOAD 512

typedef struct vits_synth_opts_watermark_payload {
  vits_synth_opts_watermark base;
  uint32_t watermark_payload;
  const uint32_t* watermark_payloads; /* NULL or [B] */
} vits_synth_opts_watermark_payload;

typedef struct stts_synth_opts_watermark_payload {
  stts_synth_opts_watermark base;
  uint32_t watermark_payload;
  const uint32_t* watermark_payloads;
} stts_synth_opts_watermark_payload;

/* Kernel-level parity doors, host buffers, the conventions of vits_op_watermark*.
 * The embed stage with one payload per item: payloads uint32 [B]; y float [B, N] as vits_op_watermark writes it. */
int vits_op_watermark_payload(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, uint32_t key, float depth_db,
                              const uint32_t* payloads, float* y);
/* The reader: z double [B] (the pilot score at the best offset), offset int32 [B] (samples, 128 o*), rows int32 [B], payload
 * uint32 [B] (W' >> 8, always reported), valid int32 [B], and, unless NULL, z_all double [B, 128] (zp_o of every offset index) and
 * bit_z double [B, 24] (z_i at o*).  An item below n/2 + 1 samples: z = 0, offset = 0, rows = 0, valid = 0. */
int vits_op_watermark_read(int device, const float* x, const int64_t* lengths, int32_t B, int64_t N, uint32_t key, double* z,
                           int32_t* offset, int32_t* rows, uint32_t* payload, int32_t* valid, double* z_all, double* bit_z);

#ifdef __cplusplus
}
#endif
#endif /* VITS_WATERMARK_PAYLOAD_H */
