"""Time greedy CTC decoding at the evaluation size of CTC pre-training (B x 375 frames x 51 867 classes, the product's 128-padded bf16
rows) against torch.argmax alone on the same tensor and against the reference's formulation (argmax, then a Python loop that reads
the device tensor element by element).  usage: python tools/bench_ctc_greedy.py [B ...]   (default: 16 48; the Python loop runs at
B = 16 only)"""
import statistics
import sys

import torch

sys.path.insert(0, ".")
import amd_pkg
pkg = amd_pkg.load()

Tn, V1, LD = 375, 51867, 51968
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12           # bytes / s: the HBM3E figure and the measured float4 copy rate of the MI355X
ROUNDS, CALLS = 9, 10


def timed(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3         # us per call


def python_loop(logits, blank, pad):
    """The reference's formulation in this tool's words: every comparison below reads the device."""
    ids = torch.argmax(logits, dim=-1)
    for row in ids:
        kept, prev = [], None
        for v in row:
            if prev is None or bool(v != prev):
                if bool(v != blank):
                    kept.append(v)
                prev = v
        n = len(kept)
        if n:
            row[:n] = torch.stack(kept)
        row[n:] = pad
    return ids


def spread(xs):
    return f"median {statistics.median(xs):.1f} us (min {min(xs):.1f}, max {max(xs):.1f} over {len(xs)} rounds of {CALLS} calls)"


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [16, 48]
    print(f"tools/bench_ctc_greedy.py: Tn={Tn}, V1={V1}, bf16 rows of {LD}; (a) ctc_greedy_decode and (b) torch.argmax(logits[..., :V1], -1) "
          f"alternate for {ROUNDS} rounds after a warm-up of both")
    for B in sizes:
        buf = torch.zeros(B, Tn, LD, dtype=torch.bfloat16, device="cuda")
        logits = buf[:, :, :V1]
        logits.copy_(torch.randn(B, Tn, V1, dtype=torch.bfloat16, device="cuda") * 3)
        path = torch.randint(0, V1, (B, Tn // 3 + 1), device="cuda").repeat_interleave(3, dim=1)[:, :Tn]      # runs of three frames
        path[:, ::7] = V1 - 1                                                                                 # and blanks
        logits.scatter_(2, path[:, :, None], 20.0)
        blank, pad = V1 - 1, 50257
        a = lambda: pkg.ctc_greedy_decode(logits, blank, pad)            # noqa: E731
        b = lambda: torch.argmax(logits, dim=-1)                         # noqa: E731
        got = a()
        want = python_loop(logits[:1], blank, pad)
        assert torch.equal(got[:1], want) and torch.equal(b(), path), "the decoders disagree"
        timed(a, 3), timed(b, 3)
        ta, tb = [], []
        for _ in range(ROUNDS):
            ta.append(timed(a, CALLS))
            tb.append(timed(b, CALLS))
        need = B * Tn * V1 * 2
        ma = statistics.median(ta)
        print(f"B={B}: (a) ctc_greedy_decode  {spread(ta)}")
        print(f"B={B}: (b) torch.argmax alone {spread(tb)}")
        print(f"B={B}: (a) must read {need / 1e6:.1f} MB -> {need / ma / 1e6:.2f} TB/s = {100 * need / (ma * 1e-6) / HBM_SPEC:.0f} % of the 8.0 TB/s HBM3E figure, "
              f"{100 * need / (ma * 1e-6) / HBM_COPY:.0f} % of the measured 6.29 TB/s copy rate; (a) - (b) = {ma - statistics.median(tb):+.1f} us, "
              f"spread of (b) {max(tb) - min(tb):.1f} us")
        if B == 16:
            tc = [timed(lambda: python_loop(logits, blank, pad), 1) for _ in range(2)]
            print(f"B={B}: (c) argmax + Python loop over the device tensor: {tc[0] / 1e3:.0f} ms, {tc[1] / 1e3:.0f} ms (2 calls) -> {min(tc) / ma:.0f} x (a)")
        del buf, logits


if __name__ == "__main__":
    main()
