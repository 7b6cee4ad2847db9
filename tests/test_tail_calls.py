"""Every call that reaches the C ABI for the request matrix of tools/tail_calls.py (sessions, coalescer and MultiDeviceSynth around a
recorder that stands where the library stands) equals tests/golden/tail_calls.txt line for line: entry point, struct class and size,
flags, fields, the order of the host doors, and the type and message of every refusal.  The golden is the tool's output for the commit
before the Python tail was folded into outopts.Tail; a feature that adds a stage extends the matrix and the golden in one diff."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def test_every_call_at_the_c_abi_equals_the_recorded_one():
    sys.path.insert(0, os.path.join(HERE, "..", "tools"))
    try:
        import tail_calls
    finally:
        sys.path.pop(0)
    got = tail_calls.dump().splitlines()
    with open(os.path.join(HERE, "golden", "tail_calls.txt")) as f:
        want = f.read().splitlines()
    label = None
    for n, (g, w) in enumerate(zip(got, want), 1):
        if w.startswith("== "):
            label = w
        assert g == w, f"line {n} (request {label}):\n  golden: {w}\n  now:    {g}"
    assert len(got) == len(want), f"{len(got)} lines now, {len(want)} in the golden"
    assert len(want) > 1000 and sum(w.startswith("!! ") for w in want) > 50  # (the matrix ran: requests and refusals both)
