// Host-side check of the output tail's request parsing (vosk_tts_amd/csrc/out_tail.hip.h: tail_fields_vits / tail_fields_stts /
// tail_req), which needs no device.  A stand-alone program: build it with the host sanitizers and run it,
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/out_tail_hostcheck.hip -o tools/out_tail_hostcheck && tools/out_tail_hostcheck
//
// The extended option structs of include/vits_{loudness,pitch,limit}.h are a chain of `base` members, and a field is read under its own
// flag alone: a caller who sets no flag of an extension passes the shorter struct.  So for every flag combination and every struct of
// the chain long enough for it, the options are copied into a heap block of exactly sizeof(that struct) -- a read beyond it lands in
// the sanitizer's red zone -- and the fields and the request that come back are compared with what went in.  Not part of the test
// suite: nothing here touches the GPU, and nothing is loaded into Python.
#include "../vosk_tts_amd/csrc/engine.hip"

extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }  // (the HIP runtime's own start-up allocations)

static int g_checks = 0, g_bad = 0;
#define CHECK(c)                                                             \
  do {                                                                       \
    ++g_checks;                                                              \
    if (!(c)) { ++g_bad; printf("FAILED line %d: %s\n", __LINE__, #c); }     \
  } while (0)

static float g_loud[2], g_gain[2], g_red[2];

// the flags of a combination in the family's own bits
static uint32_t flag_bits(const TailFamily& fam, int combo) {
  return (combo & 1 ? fam.loudness : 0) | (combo & 2 ? fam.pitch : 0) | (combo & 4 ? fam.formant : 0) | (combo & 8 ? fam.limit : 0);
}

template <typename Loud>
static void fill_loud(Loud* o) { o->loudness_mode = VITS_LOUDNESS_LUFS; o->loudness_target = -19.f; o->loudness_ceiling = 0.f; o->out_loudness = g_loud; o->out_gain = g_gain; }
template <typename Limit>
static void fill_limit(Limit* o) {
  o->limit_mode = VITS_LIMIT_TRUE; o->limit_ceiling = 0.8f; o->limit_lookahead_ms = 4.f; o->limit_release_ms = 60.f; o->limit_gain = 1.5f; o->out_reduction = g_red;
}

static void check_fields(const TailFields& f, int combo, const char* family) {
  CHECK(!strcmp(f.family, family));
  CHECK(f.loud_on == !!(combo & 1) && f.pitch_on == !!(combo & 2) && f.formant == !!(combo & 4) && f.lim_on == !!(combo & 8));
  if (f.loud_on) CHECK(f.loud_mode == VITS_LOUDNESS_LUFS && f.loud_target == -19.f && f.loud_ceiling == 0.f && f.out_loudness == g_loud && f.out_gain == g_gain);
  else CHECK(f.loud_mode == 0 && f.loud_target == 0.f && !f.out_loudness && !f.out_gain);
  if (f.pitch_on) CHECK(f.semitones == 3.f);
  else CHECK(f.semitones == 0.f);
  if (f.lim_on) CHECK(f.lim_mode == VITS_LIMIT_TRUE && f.lim_ceiling == 0.8f && f.lim_lookahead_ms == 4.f && f.lim_release_ms == 60.f && f.lim_gain == 1.5f && f.out_reduction == g_red);
  else CHECK(f.lim_mode == 0 && f.lim_ceiling == 0.f && !f.out_reduction);
}

// what tail_req makes of a combination at `sample_rate`, for a vocoder at 22050 Hz / hop 256
static void check_req(const vits_model* v, const TailFields& f, int combo, int32_t sample_rate) {
  for (int pcm = 0; pcm < 2; ++pcm) {
    TailReq q;
    const int rc = tail_req(v, f, sample_rate, pcm != 0, pcm ? 0.9f : 1.f, &q);
    if ((combo & 4) && !(combo & 2)) {  // the formant bit alone: refused, in the family's own words
      CHECK(rc == VITS_ERR_ARG && strstr(vits_last_error(), f.family) == vits_last_error() && strstr(vits_last_error(), "_FLAG_PITCH_FORMANT without"));
      continue;
    }
    CHECK(rc == VITS_OK);
    CHECK(q.pcm == (pcm != 0) && q.pcm_scale == (pcm ? 0.9f : 1.f) && q.T == nullptr);
    CHECK(q.rate == (sample_rate == 22050 ? 0 : sample_rate));
    const int hz = q.rate ? q.rate : 22050;
    CHECK(q.norm.loud.on == !!(combo & 1) && q.norm.lim.on == !!(combo & 8) && q.pitch.on == !!(combo & 2));
    if (q.norm.loud.on) CHECK(q.norm.loud.P.rate == hz && q.norm.loud.prm.target == -19.f && q.norm.loud.out_loudness == g_loud && q.norm.loud.out_gain == g_gain);
    if (q.norm.lim.on) CHECK(q.norm.lim.rate == hz && q.norm.lim.out_reduction == g_red && q.norm.lim.prm.mode == VITS_LIMIT_TRUE);
    if (q.pitch.on) CHECK(q.pitch.semitones == 3.f && q.pitch.formant == !!(combo & 4) && q.pitch.P != q.pitch.Q);
  }
}

// One family: `opts` is the longest struct of its chain, filled; sizes[] the chain from the plain struct up; need(combo) the index of
// the shortest struct that carries every field the combination reads.
template <typename Plain, typename Full, typename Fields, typename Need>
static void run_family(const vits_model* v, const TailFamily& fam, const Full& opts, const size_t* sizes, int n_sizes, Fields fields, Need need) {
  for (int combo = 0; combo < 16; ++combo)
    for (int k = need(combo); k < n_sizes; ++k) {
      char* blk = static_cast<char*>(malloc(sizes[k]));  // exactly the struct: what lies behind it is the red zone
      memcpy(blk, &opts, sizes[k]);
      reinterpret_cast<Plain*>(blk)->flags = flag_bits(fam, combo);
      const TailFields f = fields(reinterpret_cast<const Plain*>(blk));
      free(blk);
      check_fields(f, combo, fam.name);
      for (int32_t rate : {0, 22050, 16000}) check_req(v, f, combo, rate);
    }
  const TailFields none = fields(nullptr);  // no options at all
  check_fields(none, 0, fam.name);
}

int main() {
  vits_model* v = new vits_model();  // (never freed: only its hparams are read)
  v->hp.sampling_rate = 22050;
  v->hp.hop_length = 256;

  vits_synth_opts_limit vo;
  memset(&vo, 0, sizeof(vo));
  fill_loud(&vo.base.base);
  vo.base.pitch_semitones = 3.f;
  fill_limit(&vo);
  const size_t vs[] = {sizeof(vits_synth_opts), sizeof(vits_synth_opts_pitch), sizeof(vits_synth_opts_limit)};
  run_family<vits_synth_opts>(v, TAIL_VITS, vo, vs, 3, tail_fields_vits, [](int c) { return c & 8 ? 2 : c & 2 ? 1 : 0; });

  stts_synth_opts_limit so;
  memset(&so, 0, sizeof(so));
  fill_loud(&so.base.base);
  so.base.pitch_semitones = 3.f;
  fill_limit(&so);
  const size_t ss[] = {sizeof(stts_synth_opts), sizeof(stts_synth_opts_loudness), sizeof(stts_synth_opts_pitch), sizeof(stts_synth_opts_limit)};
  run_family<stts_synth_opts>(v, TAIL_STTS, so, ss, 4, tail_fields_stts, [](int c) { return c & 8 ? 3 : c & 2 ? 2 : c & 1 ? 1 : 0; });

  // the refusals tail_req makes itself, in the order rate, loudness, limit, pitch; and a model without a vocoder
  TailReq q;
  vo.base.base.flags = flag_bits(TAIL_VITS, 1 | 2 | 8);
  TailFields f = tail_fields_vits(&vo.base.base);
  CHECK(tail_req(v, f, 7, false, 1.f, &q) != VITS_OK);  // no plan for 22050 -> 7 Hz
  f.loud_ceiling = 0.9f;
  CHECK(tail_req(v, f, 0, false, 1.f, &q) == VITS_ERR_ARG && strstr(vits_last_error(), "loudness_ceiling 0.9 with the limit flag"));
  f.loud_ceiling = 0.f;
  f.semitones = 13.f;
  CHECK(tail_req(v, f, 0, false, 1.f, &q) == VITS_ERR_ARG && strstr(vits_last_error(), "pitch: 13 semitones outside"));
  f.semitones = 0.f;  // the identity: the call as it was
  CHECK(tail_req(v, f, 0, false, 1.f, &q) == VITS_OK && !q.pitch.on && q.norm.loud.on && q.norm.lim.on);
  CHECK(tail_req(nullptr, f, 0, false, 1.f, &q) == VITS_ERR_ARG && !strcmp(vits_last_error(), "no vocoder attached"));
  CHECK(tail_req(nullptr, TailFields(), 16000, false, 1.f, &q) == VITS_OK && q.rate == 16000 && !q.norm.on() && !q.pitch.on);
  // the stream refusals name the family
  CHECK(tail_refuse_stream(0, TAIL_VITS) == VITS_OK && tail_refuse_stream(VITS_FLAG_SOLO_BATCH, TAIL_VITS) == VITS_OK);
  CHECK(tail_refuse_stream(STTS_FLAG_LIMIT, TAIL_STTS) == VITS_ERR_UNSUPPORTED && strstr(vits_last_error(), "STTS_FLAG_LIMIT on a stream") == vits_last_error());
  CHECK(tail_refuse_stream(VITS_FLAG_PITCH, TAIL_VITS) == VITS_ERR_UNSUPPORTED && strstr(vits_last_error(), "VITS_FLAG_PITCH on a stream") == vits_last_error());

  printf("out_tail_hostcheck: %d checks, %d failed\n", g_checks, g_bad);
  return g_bad ? 1 : 0;
}
