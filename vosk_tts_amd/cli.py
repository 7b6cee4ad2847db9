#!/usr/bin/env python3
"""Console entry point with the flag surface of the reference `vosk-tts` script (vosk_tts/cli.py:12-43):
-m/--model, -n/--model-name, -l/--lang, -i/--input, -s/--speaker, -r/--speech-rate, -o/--output,
--list-models, --list-languages, --log-level.  Behaviour mirrored from cli.py:45-65: listing flags
short-circuit, a missing --input logs a hint and exits with status 1, otherwise one utterance is
synthesised to a 22.05 kHz mono 16-bit WAV through the MI355X engine.

    python -m vosk_tts_amd.cli -m /path/to/model-dir -i "прив+ет м+ир" -s 2 -o out.wav
"""
import argparse
import json
import logging
import sys

# (flags, argparse keyword arguments) — one row per option of the reference CLI, plus --sample-rate (tts_service.proto's
# output_audio_spec.raw_audio.sample_rate_hertz; the reference script has no such flag) and --denoiser-strength (the
# --denoiser_strength of the StableTTS script, training/stabletts/matcha/cli.py:253-256)
_OPTIONS = (
    (("-m", "--model"), dict(type=str, metavar="DIR", help="directory holding model.vitsw, dictionary and config.json")),
    (("-n", "--model-name"), dict(type=str, metavar="NAME", help="pick a locally installed model by its directory name")),
    (("-l", "--lang"), dict(type=str, default="en-us", metavar="LANG", help="pick a locally installed model by language code")),
    (("-i", "--input"), dict(type=str, metavar="TEXT", help="text to speak ('+' marks the stressed vowel)")),
    (("-s", "--speaker"), dict(type=int, metavar="ID", help="speaker index of a multi-speaker voice")),
    (("-r", "--speech-rate"), dict(type=float, default=1.0, metavar="X", help="tempo multiplier (>1 is faster)")),
    (("-o", "--output"), dict(type=str, default="out.wav", metavar="WAV", help="where to write the audio")),
    (("--list-models",), dict(action="store_true", help="print the models found in the local search path and exit")),
    (("--list-languages",), dict(action="store_true", help="print the language codes of the local models and exit")),
    (("--sample-rate",), dict(type=int, default=None, metavar="HZ", help="output sample rate (default: the voice's own, 22050)")),
    (("--denoiser-strength",), dict(type=float, default=None, metavar="S",
                                    help="vocoder-bias denoiser of a multistream voice (the StableTTS script's default is 0.00025; default here: "
                                         "the voice's inference.denoiser_strength, else off)")),
    (("--loudness",), dict(type=float, default=None, metavar="LUFS",
                           help="normalise the audio to this ITU-R BS.1770 integrated loudness, e.g. -19 (default: the voice's "
                                "inference.loudness, else off)")),
    (("--peak",), dict(type=float, default=None, metavar="P",
                       help="normalise the audio to this peak in (0, 1] instead (not together with --loudness)")),
    (("--limit",), dict(choices=("sample", "true"), default=None,
                        help="look-ahead peak limiter on sample peaks or on true (4x oversampled) peaks: with --loudness the target is met "
                             "and the peaks above the ceiling (the voice's inference.peak_ceiling, else 1.0) are taken down (default: the "
                             "voice's inference.limit, else off)")),
    (("--pitch",), dict(type=float, default=None, metavar="SEMITONES",
                        help="shift the pitch of the audio by this many semitones, -12 to 12, at unchanged duration (default: the voice's "
                             "inference.pitch, else none)")),
    (("--preserve-formants",), dict(action="store_true", default=None,
                                    help="with a pitch shift: keep the voice's formants where they were (default: the voice's "
                                         "inference.pitch_formants, else off)")),
    (("--duration",), dict(type=float, default=None, metavar="SECONDS",
                           help="speak the text in this many seconds: the durations are fitted to round(SECONDS * rate / hop) frames in one pass")),
    (("--pause",), dict(action="append", default=None, metavar="INDEX:SECONDS",
                        help="a pause of SECONDS behind word INDEX (counted from 0); repeatable")),
    (("--word-rate",), dict(action="append", default=None, metavar="INDEX:RATE",
                            help="speak word INDEX at RATE times the tempo (>1 is faster); repeatable")),
    (("--word-pitch",), dict(action="append", default=None, metavar="INDEX=SEMITONES",
                             help="raise or lower word INDEX by SEMITONES, -12 to 12, at unchanged duration; repeatable")),
    (("--word-gain",), dict(action="append", default=None, metavar="INDEX=DB",
                            help="speak word INDEX DB decibels louder (-40 to 12); repeatable")),
    (("--pitch-range",), dict(type=float, default=None, metavar="R",
                              help="intonation range: how far the voice moves about its median pitch, 0 (monotone) to 4, 1 = unchanged")),
    (("--watermark",), dict(type=lambda text: _key(text), default=None, metavar="KEY",
                            help="mark the audio with this 32-bit key (decimal or 0x...), a +-1 dB spectral ripple that --detect-watermark "
                                 "recognises; a selector, not a secret")),
    (("--detect-watermark",), dict(type=str, default=None, metavar="FILE",
                                   help="instead of synthesising: look for the mark of --watermark KEY (default: the voice's "
                                        "inference.watermark_key) in this 16-bit mono WAV and print detected, z and the offset in samples")),
    (("--watermark-payload",), dict(type=int, default=None, metavar="N",
                                    help="with --watermark: carry N, 0 to 65535, inside the mark (2 dB deep by default); --read-watermark returns it")),
    (("--read-watermark",), dict(type=str, default=None, metavar="FILE",
                                 help="instead of synthesising: read the mark of --watermark KEY (default: the voice's inference.watermark_key) "
                                      "in this 16-bit mono WAV and print detected, z, the offset in samples, the payload (null unless valid) "
                                      "and the weakest coded bit's score")),
    (("--locate-watermark",), dict(type=str, default=None, metavar="FILE",
                                   help="instead of synthesising: find where the mark of --watermark KEY (default: the voice's "
                                        "inference.watermark_key) sits in this 16-bit mono WAV and print one line per marked segment, in seconds")),
    (("--watermark-span",), dict(type=int, default=4, metavar="N",
                                 help="with --locate-watermark: pattern periods per scored window, 1 to 8 (default 4; a period is 16384 samples)")),
    (("--read-payload",), dict(action="store_true",
                               help="with --locate-watermark: the audio was marked with --watermark-payload; also read each segment's payload")),
    (("--ssml",), dict(action="store_true", help="the input is an SSML document: speak, p, s, sub, break, prosody, mark")),
    (("--document",), dict(action="store_true",
                           help="the input is a document: split into sentences and paragraphs (blank lines), synthesised as one batch and "
                                "joined on the device, so --loudness / --limit see the whole output; with --ssml: s, p and voice end segments")),
    (("--sentence-pause",), dict(type=float, default=0.2, metavar="SECONDS", help="with --document: silence behind a sentence (default 0.2)")),
    (("--paragraph-pause",), dict(type=float, default=0.6, metavar="SECONDS", help="with --document: silence behind a paragraph (default 0.6)")),
    (("--trim-db",), dict(type=float, default=None, metavar="DBFS",
                          help="with --document: cut the frames below this level, e.g. -50, from both ends of every sentence (default: off)")),
    (("--marks",), dict(type=str, default=None, metavar="FILE",
                        help="also write the speech marks as JSON: rate, phonemes and words with their offsets in samples and seconds")),
    (("--log-level",), dict(default="INFO", metavar="LEVEL", help="python logging level (INFO shows the RTF line)")),
)


def _key(text):
    """a watermark key on the command line: decimal or 0x-prefixed, in [0, 2^32)"""
    try:
        k = int(text, 0)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r}: a key is an integer, decimal or 0x...")
    if not 0 <= k < 1 << 32:
        raise argparse.ArgumentTypeError(f"key {k} outside [0, 2^32)")
    return k


def _wav_pcm(path, flag):
    import wave

    import numpy as np

    with wave.open(path, "r") as f:
        if f.getsampwidth() != 2 or f.getnchannels() != 1:
            raise SystemExit(f"{flag} {path}: a 16-bit mono WAV is expected")
        return np.frombuffer(f.readframes(f.getnframes()), np.int16)


def detect_watermark(synth, path, key):
    """--detect-watermark: the triple of Synth.detect_watermark for a 16-bit mono WAV, printed as one JSON line"""
    detected, z, offset = synth.detect_watermark(_wav_pcm(path, "--detect-watermark"), key)
    print(json.dumps({"detected": detected, "z": round(z, 3), "offset_samples": offset}))
    return 0


def read_watermark(synth, path, key):
    """--read-watermark: Synth.read_watermark for a 16-bit mono WAV, printed as one JSON line"""
    detected, z, offset, payload, bit_z = synth.read_watermark(_wav_pcm(path, "--read-watermark"), key)
    print(json.dumps({"detected": detected, "z": round(z, 3), "offset_samples": offset, "payload": payload,
                      "min_abs_bit_z": round(float(abs(bit_z).min()), 3)}))
    return 0


def locate_watermark(synth, path, key, span=4, payload=False):
    """--locate-watermark: Synth.locate_watermark for a 16-bit mono WAV, one JSON line per segment, in seconds of the file's own rate"""
    import wave

    with wave.open(path, "r") as f:
        rate = f.getframerate()
    for s in synth.locate_watermark(_wav_pcm(path, "--locate-watermark"), key, span=span, payload=payload):
        line = {"start_s": round(s.start / rate, 3), "end_s": round(s.end / rate, 3), "z": round(s.z, 3), "offset_samples": s.offset_samples}
        if payload:
            line["payload"] = s.payload
        print(json.dumps(line))
    return 0


def build_parser():
    ap = argparse.ArgumentParser(prog="vosk-tts-amd", description="Text to speech on the MI355X-native VITS2 engine")
    for flags, kw in _OPTIONS:
        ap.add_argument(*flags, **kw)
    return ap


def _indexed(pairs, flag, sep=":"):
    """["INDEX:VALUE", ...] of a repeatable flag -> {index: value}, or None"""
    if not pairs:
        return None
    out = {}
    for p in pairs:
        try:
            k, v = p.split(sep, 1)
            out[int(k)] = float(v)
        except ValueError:
            raise SystemExit(f"{flag} {p!r}: expected INDEX{sep}VALUE, e.g. 0{sep}0.5")
    return out


def run(opts):
    from . import model as model_mod

    logging.getLogger().setLevel(opts.log_level.upper())
    for wanted, action in ((opts.list_models, model_mod.list_models), (opts.list_languages, model_mod.list_languages)):
        if wanted:
            action()
            return 0
    detect = getattr(opts, "detect_watermark", None)
    read = getattr(opts, "read_watermark", None)
    if getattr(opts, "watermark_payload", None) is not None and getattr(opts, "watermark", None) is None:
        raise SystemExit("--watermark-payload needs --watermark KEY")
    locate = getattr(opts, "locate_watermark", None)
    if not opts.input and not detect and not read and not locate:
        logging.info("Please specify input text or file")
        return 1
    from .synth import Synth

    voice = model_mod.Model(opts.model, opts.model_name, opts.lang)
    synth = Synth(voice)
    if detect:
        return detect_watermark(synth, detect, getattr(opts, "watermark", None))
    if read:
        return read_watermark(synth, read, getattr(opts, "watermark", None))
    if locate:
        return locate_watermark(synth, locate, getattr(opts, "watermark", None), getattr(opts, "watermark_span", 4),
                                bool(getattr(opts, "read_payload", False)))
    wm = {} if getattr(opts, "watermark", None) is None else {"watermark": opts.watermark}
    if getattr(opts, "watermark_payload", None) is not None:
        wm["watermark_payload"] = opts.watermark_payload
    if getattr(opts, "document", False):  # many sentences in one call (Synth.synth_document); the per-word flags index one utterance
        import wave

        for flag in ("duration", "pause", "word_rate", "word_pitch", "word_gain"):
            if getattr(opts, flag, None) is not None:
                raise SystemExit(f"--{flag.replace('_', '-')} indexes the words of one utterance: not with --document")
        fn = synth.synth_document_ssml if getattr(opts, "ssml", False) else synth.synth_document
        res = fn(opts.input, speaker_id=opts.speaker or 0, sentence_pause=opts.sentence_pause, paragraph_pause=opts.paragraph_pause,
                 trim_db=opts.trim_db, speech_rate=opts.speech_rate, sample_rate=opts.sample_rate, denoiser_strength=opts.denoiser_strength,
                 marks=bool(opts.marks), loudness=opts.loudness, peak=opts.peak, pitch=opts.pitch, preserve_formants=opts.preserve_formants,
                 **({} if opts.limit is None else {"limit": opts.limit}),
                 **({} if getattr(opts, "pitch_range", None) is None else {"pitch_range": opts.pitch_range}), **wm)
        audio, marks = res if opts.marks else (res, None)
        with wave.open(opts.output, "w") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(int(opts.sample_rate) if opts.sample_rate else synth.native_rate())
            f.writeframes(audio.tobytes())
        if opts.marks:
            with open(opts.marks, "w", encoding="utf-8") as f:
                f.write(json.dumps(dict(marks.to_dict(), segments=[{"start_sample": a, "end_sample": b} for a, b in marks.segments]),
                                   ensure_ascii=False, indent=1) + "\n")
        return 0
    if getattr(opts, "ssml", False):  # the document's markup takes the place of the per-word flags
        import wave

        res = synth.synth_ssml(opts.input, speaker_id=opts.speaker, speech_rate=opts.speech_rate, sample_rate=opts.sample_rate,
                               denoiser_strength=opts.denoiser_strength, marks=bool(opts.marks), loudness=opts.loudness, peak=opts.peak,
                               pitch=opts.pitch, **({} if opts.limit is None else {"limit": opts.limit}),
                               **({} if getattr(opts, "pitch_range", None) is None else {"pitch_range": opts.pitch_range}),
                               **({} if getattr(opts, "duration", None) is None else {"duration": opts.duration}), **wm)
        audio, marks = res if opts.marks else (res, None)
        with wave.open(opts.output, "w") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(int(opts.sample_rate) if opts.sample_rate else synth.native_rate())
            f.writeframes(audio.tobytes())
        if opts.marks:
            with open(opts.marks, "w", encoding="utf-8") as f:
                f.write(marks.to_json(indent=1) + "\n")
        return 0
    marks = synth.synth(opts.input, opts.output, opts.speaker, speech_rate=opts.speech_rate, sample_rate=opts.sample_rate,
                               denoiser_strength=opts.denoiser_strength, marks=bool(opts.marks), loudness=opts.loudness, peak=opts.peak, pitch=opts.pitch,
                               preserve_formants=opts.preserve_formants, **({} if opts.limit is None else {"limit": opts.limit}),
                               **{k: v for k, v in (("duration", getattr(opts, "duration", None)), ("pauses", _indexed(getattr(opts, "pause", None), "--pause")),
                                                    ("word_rates", _indexed(getattr(opts, "word_rate", None), "--word-rate")),
                                                    ("word_pitch", _indexed(getattr(opts, "word_pitch", None), "--word-pitch", "=")),
                                                    ("word_gains", _indexed(getattr(opts, "word_gain", None), "--word-gain", "=")),
                                                    ("pitch_range", getattr(opts, "pitch_range", None))) if v is not None}, **wm)
    if opts.marks:
        with open(opts.marks, "w", encoding="utf-8") as f:
            f.write(marks.to_json(indent=1) + "\n")
    return 0


def main(argv=None):
    status = run(build_parser().parse_args(argv))
    if status:
        sys.exit(status)


if __name__ == "__main__":
    main()
