#!/usr/bin/env python3
"""Recorded results of the decoder's host arithmetic (tests/golden/decoder_geom.json), read from the product library as it stands:
for the 43 rows of tests/decoder_grid.py and the default / multistream / single-band / plain-Generator hparams the ragged halo
(vits_debug_rag_halo) and the per-layer limits (vits_debug_decoder_needs); the same two hooks' answers for the nine refused
geometries; and, with --device (needs a GPU: both take a created model), per grid row vits_algorithmic_flops(1, 1, 0) / (1, 0, 1)
and per refused geometry vits_create's error code and message.  Run it BEFORE a change that must leave these values alone:

    python tools/gen_golden_decoder_geom.py            # host part (keeps a device part already recorded)
    python tools/gen_golden_decoder_geom.py --device   # both parts
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

from decoder_grid import GRID, REFUSED, refused_hparams, row_hparams  # noqa: E402
from vosk_tts_amd import weights as W  # noqa: E402
from vosk_tts_amd.capi import VitsError, VitsLib  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "decoder_geom.json")
NAMED = {"default": W.default_hparams, "multistream": W.multistream_hparams, "istft": W.istft_hparams, "plain": W.plain_hparams}


def hooks(lib, hp):
    """{"rag_halo": ..., "needs": ...}: the hooks' values, or the error code a hook answers with"""
    out = {}
    for key, fn in (("rag_halo", lib.rag_halo), ("needs", lib.decoder_needs)):
        try:
            out[key] = fn(hp)
        except VitsError as e:
            out[key] = {"error": e.code}
    return out


def main():
    lib = VitsLib()
    doc = json.load(open(OUT)) if os.path.exists(OUT) else {}
    doc["rows"] = {r[0]: hooks(lib, row_hparams(r)) for r in GRID}
    doc["rows"].update({k: hooks(lib, f()) for k, f in NAMED.items()})
    doc["refused"] = {e[0]: hooks(lib, refused_hparams(e)) for e in REFUSED}
    if "--device" in sys.argv[1:]:
        doc["flops"], doc["refusals"] = {}, {}
        for r in GRID:
            hp = row_hparams(r)
            m = lib.create(W.pack_blob(hp, W.make_synthetic_weights(hp, 1234)), 0)
            doc["flops"][r[0]] = [m.algorithmic_flops(1, 1, 0), m.algorithmic_flops(1, 0, 1)]
            m.close()
        for e in REFUSED:
            hp = refused_hparams(e)
            try:
                lib.create(W.pack_blob(hp, W.make_synthetic_weights(hp, 1234), validate=False), 0).close()
                doc["refusals"][e[0]] = None
            except VitsError as err:
                doc["refusals"][e[0]] = {"code": err.code, "message": str(err)}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {OUT}: {len(doc['rows'])} rows, {len(doc['refused'])} refused, device part: {'flops' in doc}")


if __name__ == "__main__":
    main()
