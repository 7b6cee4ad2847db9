/*
 * stts_bert_batch.h — padded batches of sentences through the word-embedding BERT encoder of include/stts_mi355.h.
 *
 * An extension of the product library for its batch door (vosk_tts_amd/batching.py): the reference encodes one sentence per request
 * (vosk_tts/synth.py:27-34), so the CPU oracle has no batched form and these two entry points are checked against its
 * single-sentence stts_bert_encode item by item.  Same status codes and stts_last_error as the rest of the family; both are re-entrant.
 */
#ifndef STTS_BERT_BATCH_H
#define STTS_BERT_BATCH_H

#include "stts_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ids / token_type_ids int64 [B, T] (token_type_ids may be NULL), lengths int32 [B] with 1 <= lengths[b] <= T <= max_position.
 * Entries at t >= lengths[b] are never read (they may hold anything).  out float [B, T, hidden]: rows t < lengths[b] are what
 * stts_bert_encode returns for ids[b, :lengths[b]] (positions count from 0 per item, keys masked at the item's length); rows beyond are 0. */
int stts_bert_encode_batch(bert_model* m, const int64_t* input_ids, const int64_t* token_type_ids, const int32_t* lengths,
                           int32_t B, int32_t T, float* out);

/* The same forward, then the phoneme feed of the acoustic models without leaving the device:
 * out float [B, hidden, T_x], out[b, :, t] = final hidden state of token rows[b, t] of sentence b; rows[b, t] < 0 -> a zero column
 * (padding; the tokenizer-less multistream_v2 feed).  rows int32 [B, T_x]; rows[b, t] >= lengths[b] is VITS_ERR_ARG naming b and t. */
int stts_bert_feed_batch(bert_model* m, const int64_t* input_ids, const int64_t* token_type_ids, const int32_t* lengths,
                         int32_t B, int32_t T, const int32_t* rows, int32_t T_x, float* out);

#ifdef __cplusplus
}
#endif
#endif
