"""dicow_ctc_forced_align (csrc/ctc_align.hip) against the oracle of tests/ctc_align_ref.py.

The exact cases: logits are multiples of 2^-6 in [-16, 0] with an 8-bit significand (exact in bf16 too) and lse = 0, so every sum over at
most 2048 frames is exact in fp32 and path, spans, score, token_score and status must EQUAL the integer oracle's -- the kernel has no
rounding to hide behind; 5 to 40 classes make ties frequent.  Logits, every output and the workspace live inside the guard bands of
tests/util.py::guarded; the row gap [V1, ld) and every frame outside the problems' slices hold the NaN sentinel.  Every case runs under
the library's own choice of plan and under the forced wide plan, and its problems of at most 63 targets under the forced narrow one.
Run with `pytest -m gpu`."""
import numpy as np
import pytest
import torch

import amd_pkg
from tests import ctc_align_ref as R
from tests.util import guarded, load_golden, T

pytestmark = pytest.mark.gpu
pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib as L  # noqa: E402

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
NAN = float("nan")


def dyadic(rng, shape, small=0.7):
    """Multiples of 2^-6 in [-16, 0] with at most 8 significant bits; mostly from {0 .. 7} / 64 * {1, 2, 4} so that ties abound."""
    k = np.where(rng.random(shape) < small, rng.integers(0, 8, shape), rng.integers(0, 256, shape)) << rng.integers(0, 3, shape)
    return 0.0 - k.astype(np.float64) / 64.0                                 # (0.0 - 0.0: no negative zero, whose sign the sums would keep)


def fmin(y):
    return len(y) + sum(1 for a, b in zip(y, y[1:]) if a == b)


def targets(rng, n, V1, blank, kind="random"):
    ids = [c for c in range(V1) if c != blank]
    if kind == "equal":
        return [ids[1]] * n
    if kind == "alternating":
        return [ids[j % 2] for j in range(n)]
    return [int(t) for t in rng.choice(ids, n)]


class Call:
    """One call of the entry point with everything inside guard bands.  problems: [(row, f0, F, y)]; vals fp64 [B, T, V1] (NaN outside the
    slices)."""

    def __init__(self, vals, problems, blank, dtype, *, ld=None, alias=None, lse="zeros", plan=0, Fmax=None, Lmax=None):
        B, Tn, V1 = vals.shape
        self.problems, self.blank, self.V1 = problems, blank, V1
        ld = V1 + 3 if ld is None else ld
        self.gl = guarded((B, Tn, V1), ld, dtype, strides=(Tn * ld, ld, 1), init=torch.from_numpy(vals), name="logits")
        n = len(problems)
        lens = [len(p[3]) for p in problems]
        starts = np.concatenate([[0], np.cumsum(lens)[:-1]]) if n else np.zeros(0)
        self.table = np.ascontiguousarray(np.array([(p[0], p[1], p[2], s, l) for p, s, l in zip(problems, starts, lens)], np.int64).reshape(-1, 5))
        self.flat = np.ascontiguousarray(np.array([t for p in problems for t in p[3]], np.int32))
        self.Fmax = max([p[2] for p in problems] + [1]) + 2 if Fmax is None else Fmax
        self.Lmax = max(lens + [1]) + 1 if Lmax is None else Lmax
        self.path = guarded((n, self.Fmax), self.Fmax, torch.int32, name="path")
        self.spans = guarded((n, 2 * self.Lmax), 2 * self.Lmax, torch.int32, name="spans")
        self.ts = guarded((n, self.Lmax), self.Lmax, torch.float32, name="token_score")
        self.score = guarded((n,), 1, torch.float32, name="score")
        self.status = guarded((n,), 1, torch.int32, name="status")
        lib = L.lib()
        self.need = lib.dicow_ctc_align_ws_bytes(self.table.ctypes.data, n)
        assert self.need > 0 and self.need % 16 == 0
        self.ws = guarded((self.need // 4,), 1, torch.int32, name="ws")
        assert self.ws.view.data_ptr() % 16 == 0
        self.lse = torch.zeros(B * Tn, device="cuda") if isinstance(lse, str) and lse == "zeros" else lse
        self.alias = None if alias is None else torch.tensor(alias, dtype=torch.int32, device="cuda")
        self.args = (self.gl.view.data_ptr(), int(dtype == torch.bfloat16), B, Tn, V1, ld, L.ptr(self.lse), L.ptr(self.alias), blank,
                     self.table.ctypes.data, n, self.flat.ctypes.data if len(self.flat) else None, len(self.flat), self.path.view.data_ptr(),
                     self.Fmax, self.spans.view.data_ptr(), self.Lmax, self.ts.view.data_ptr(), self.score.view.data_ptr(),
                     self.status.view.data_ptr(), plan, self.ws.view.data_ptr(), self.need)

    def launch(self):
        L.call("dicow_ctc_forced_align", *self.args, L.stream())

    def results(self):
        torch.cuda.synchronize()
        for g in (self.gl, self.path, self.spans, self.ts, self.score, self.status, self.ws):
            g.check()
        for g in (self.path, self.spans, self.ts, self.score, self.status):
            assert g.untouched_inside() == 0, g.name                         # every element of every output was written
        return dict(path=self.path.view.cpu(), spans=self.spans.view.cpu().view(-1, self.Lmax, 2), token_score=self.ts.view.cpu(),
                    score=self.score.view.cpu(), status=self.status.view.cpu())


def expected(vals, problems, blank, Fmax, Lmax, alias=None):
    """The integer oracle on 64 x the values (alias applied to the columns), laid out as the kernel's outputs."""
    n = len(problems)
    out = dict(path=torch.full((n, Fmax), -1, dtype=torch.int32), spans=torch.full((n, Lmax, 2), -1, dtype=torch.int32),
               token_score=torch.zeros(n, Lmax), score=torch.zeros(n), status=torch.zeros(n, dtype=torch.int32))
    for i, (row, f0, F, y) in enumerate(problems):
        x = vals[row, f0:f0 + F]
        if alias is not None:
            x = x[:, alias]
        assert not np.isnan(x).any()
        xi = np.where(np.isinf(x), float(R.NEG_INT), x * 64.0)
        assert np.array_equal(xi, np.round(xi))
        r = R.align(xi.astype(np.int64), y, blank)
        out["status"][i] = r["status"]
        out["score"][i] = r["score"] / 64.0 if r["status"] == 0 else -np.inf
        if r["status"] == 0:
            R.check_path(r["path"], y, blank)
            out["path"][i, :F] = torch.tensor(r["path"], dtype=torch.int32)
            if y:
                out["spans"][i, :len(y)] = torch.tensor(r["spans"], dtype=torch.int32)
                out["token_score"][i, :len(y)] = torch.tensor([t / 64.0 for t in r["token_score"]])
    return out


def bits_equal(a, b):
    return all(torch.equal(a[k].contiguous().view(torch.int32), b[k].contiguous().view(torch.int32)) for k in a)


def layout(rng, shapes, B, Tn, V1, blank, kinds=None):
    """Problems of the given (L, F) on rows permuted and repeated, at random f0; values NaN outside the slices."""
    vals = np.full((B, Tn, V1), NAN)
    problems = []
    for k, (Ln, F) in enumerate(shapes):
        row = int(rng.integers(0, B)) if k % 3 else (B - 1 - k // 3) % B
        f0 = int(rng.integers(0, Tn - F + 1))
        problems.append((row, f0, F, targets(rng, Ln, V1, blank, (kinds or {}).get(k, "random"))))
        blk = vals[row, f0:f0 + F]
        blk[np.isnan(blk)] = dyadic(rng, blk.shape)[np.isnan(blk)]
    return vals, problems


def run_exact(vals, problems, blank, dt, plan, finite=True, **kw):
    if plan == 1:
        problems = [p for p in problems if len(p[3]) <= 63]
    c = Call(vals, problems, blank, DT[dt], plan=plan, **kw)
    c.launch()
    got, want = c.results(), expected(vals, problems, blank, c.Fmax, c.Lmax, kw.get("alias"))
    if finite:                                                               # without -inf a problem is infeasible exactly when its frames are too few
        assert want["status"].tolist() == [int(p[2] < fmin(p[3])) for p in problems]
    for k in ("status", "score", "path", "spans", "token_score"):
        bad = [i for i in range(len(problems)) if not torch.equal(got[k][i], want[k][i])]
        assert not bad, (k, [(i, len(problems[i][3]), problems[i][2]) for i in bad[:5]], got[k][bad[0]], want[k][bad[0]])
    assert bits_equal(got, want)
    return got


PLANS = [0, 1, 2]


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("dt", list(DT))
def test_lane_ownership_edges(dt, plan):
    """L at the edges of a lane's states (8 labels a lane wide: 7 8 9, 15 16 17, 31 32 33) and of the narrow plan (63 | 64 65); F = 1, L, one
    below the minimum feasible (status 1), the minimum, and a few more; one call, rows permuted and repeated, f0 > 0."""
    rng = np.random.default_rng(100)
    V1, blank = 5, 2
    shapes = []
    for Ln in (0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65):
        for F in sorted({1, max(Ln, 1), 2 * Ln - Ln // 2, 2 * Ln + 3}):
            shapes.append((Ln, F))
    vals, problems = layout(rng, shapes, 4, 160, V1, blank)
    # exactly the minimum feasible F and one below it, for the targets as drawn
    more = []
    for row, f0, F, y in problems:
        for F2 in (fmin(y), fmin(y) - 1):
            if 0 <= F2 <= 160 - f0 and not np.isnan(vals[row, f0:f0 + F2]).any():
                more.append((row, f0, F2, y))
    got = run_exact(vals, problems + more, blank, dt, plan)
    assert 0 < int(got["status"].sum()) < len(got["status"])


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("dt", list(DT))
def test_staging_block_edges_and_sizes_side_by_side(dt, plan):
    """F around the walk's 64-frame blocks of back-pointers (row 0 holds none: 64 65 66 as well as 63), one and several blocks, next to
    problems of one frame and of no target; all-equal and alternating targets."""
    rng = np.random.default_rng(101)
    V1, blank = 7, 6
    shapes = [(Ln, F) for Ln in (3, 70) for F in (63, 64, 65, 66, 127, 128, 129, 130, 200) if F >= Ln]
    shapes += [(0, 1), (0, 129), (1, 1)]
    kinds = {}
    for Ln, F, kind in ((30, 58, "equal"), (30, 59, "equal"), (30, 200, "equal"), (31, 30, "alternating"), (31, 31, "alternating"),
                        (31, 64, "alternating"), (40, 79, "equal"), (90, 178, "equal"), (90, 179, "equal")):
        kinds[len(shapes)] = kind                                            # n equal targets need 2 n - 1 frames, n alternating ones n
        shapes.append((Ln, F))
    vals, problems = layout(rng, shapes, 3, 260, V1, blank, kinds)
    got = run_exact(vals, problems, blank, dt, plan)
    assert {0, 1} == set(got["status"].tolist())                             # (which is which: run_exact, from the frames each needs)


@pytest.mark.parametrize("dt", list(DT))
def test_the_longest_targets_and_2048_frames(dt):
    """L = 511 (1023 states: every lane of the wide plan, its last state unused), at the minimum feasible F, one below it and well above;
    2048 frames, where the exact sums end; V1 = 40."""
    rng = np.random.default_rng(102)
    V1, blank = 40, 39
    y = targets(rng, 511, V1, blank)
    shapes = [(511, fmin(y) - 1), (511, fmin(y)), (511, 900), (256, 700), (20, 2048), (100, 2048)]
    vals = np.full((2, 2048, V1), NAN)
    problems = []
    for k, (Ln, F) in enumerate(shapes):
        f0 = 2048 - F if k % 2 else 0
        problems.append((k % 2, f0, F, y[:Ln]))
        blk = vals[k % 2, f0:f0 + F]
        blk[np.isnan(blk)] = dyadic(rng, blk.shape)[np.isnan(blk)]
    got = run_exact(vals, problems, blank, dt, 0, ld=48)
    assert got["status"].tolist() == [1, 0, 0, 0, 0, 0]
    with pytest.raises(L.DicowError, match="DICOW_CTC_ALIGN_MAX_L"):
        pkg.ctc_forced_align(torch.zeros(1, 600, V1, device="cuda"), [y + [1]], blank=blank, normalized=True)


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("dt", list(DT))
def test_alias_and_columns_of_minus_infinity(dt, plan):
    """alias maps ids 3 and 4 onto column 3 (adjacent targets 3 4 are different labels on one column: the skip stays open); column 5 is -inf
    in every frame: a problem that uses it is infeasible through its -inf end states; single -inf frames elsewhere are legal."""
    rng = np.random.default_rng(103)
    V1, blank = 9, 0
    alias = [0, 1, 2, 3, 3, 5, 6, 7, 8]
    vals = dyadic(rng, (2, 90, V1))
    vals[:, :, 5] = -np.inf
    vals[:, :, 4] = NAN                                                      # never read: id 4 reads column 3
    vals[0, 10:14, 1] = -np.inf
    vals[1, 40, 0] = -np.inf
    ys = [[3, 4, 3, 4, 1], [1, 5, 2], [4, 4, 3], [1, 2, 1, 2, 6, 7, 8], [5], [], [3, 4] * 20, [1] * 3]
    problems = [(k % 2, 5 * k, F, y) for k, (y, F) in enumerate(zip(ys, (5, 30, 4, 60, 9, 12, 40, 5)))]
    problems.append((0, 9, 6, [1, 2]))                                       # label 1 has frame 9 alone
    problems.append((0, 10, 4, [2, 1]))                                      # ... and no frame at all here: -inf at both end states
    got = run_exact(vals, problems, blank, dt, plan, finite=False, alias=alias)
    assert got["status"].tolist() == [0, 1, 0, 0, 1, 0, 0, 0, 0, 1]
    assert got["spans"][8, 0].tolist() == [0, 1]
    assert got["path"][0, :5].tolist() == [3, 4, 3, 4, 1]
    # the same without lse (normalized = the logits are log-probabilities) and with a non-zero lse that keeps the sums exact
    c = Call(vals, problems, blank, DT[dt], alias=alias, lse=None, plan=plan)
    c.launch()
    assert bits_equal(c.results(), expected(vals, problems, blank, c.Fmax, c.Lmax, alias))
    lse = torch.from_numpy(-dyadic(rng, (2 * 90,), small=1.0)).float()
    c = Call(vals, problems, blank, DT[dt], alias=alias, lse=lse.cuda(), plan=plan)
    c.launch()
    assert bits_equal(c.results(), expected(vals - lse.double().numpy().reshape(2, 90, 1), problems, blank, c.Fmax, c.Lmax, alias))


def test_a_problem_does_not_depend_on_its_neighbours():
    rng = np.random.default_rng(104)
    V1, blank = 6, 5
    shapes = [(int(rng.integers(0, 90)), 0) for _ in range(16)]
    shapes = [(Ln, int(rng.integers(max(2 * Ln, 1), 2 * Ln + 120))) for Ln, _ in shapes]
    vals, problems = layout(rng, shapes, 4, 300, V1, blank)
    vals[np.isnan(vals)] = dyadic(rng, vals.shape)[np.isnan(vals)]           # (one problem alone must not see NaN where its neighbours lay)
    kw = dict(Fmax=max(s[1] for s in shapes) + 2, Lmax=max(s[0] for s in shapes) + 1)
    c16 = Call(vals, problems, blank, torch.bfloat16, **kw)
    c16.launch()
    all16 = c16.results()
    c16.launch()                                                             # a second identical call
    assert bits_equal(c16.results(), all16)
    assert bits_equal(all16, expected(vals, problems, blank, c16.Fmax, c16.Lmax))
    for plan in (0, 2):
        c1 = Call(vals, problems[5:6], blank, torch.bfloat16, plan=plan, **kw)
        c1.launch()
        alone = c1.results()
        assert bits_equal(alone, {k: v[5:6] for k, v in all16.items()}), plan


def test_graph_replay():
    rng = np.random.default_rng(105)
    V1, blank = 8, 7
    vals, problems = layout(rng, [(5, 40), (70, 200), (0, 3), (12, 11), (33, 130)], 2, 220, V1, blank)
    c = Call(vals, problems, blank, torch.float32)
    want = expected(vals, problems, blank, c.Fmax, c.Lmax)
    c.launch()                                                               # (code objects load outside the capture)
    assert bits_equal(c.results(), want)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c.launch()                                                           # the table copy and two launches
    for _ in range(2):
        for g in (c.path, c.spans, c.ts, c.score, c.status, c.ws):
            g.view.fill_(7)
        graph.replay()                                                       # the replay uploads the tables again
        assert bits_equal(c.results(), want)


def test_realistic_shape_against_fp64():
    """bf16 normal logits at V1 = 51 866 in rows of 51 968, F = 375 and F = 1500, L = 40, the device's own lse copied back so that the oracle
    sees the kernel's x.  The kernel's path must spell the targets; |score - best64| and best64 - (the kernel's path re-scored in fp64) stay
    under F^2 max|x| 2^-24: every add rounds by at most 2^-24 |v| and |v| <= F max|x|.  Measured on an MI355X (profiles/ctc_align.txt):
    the gaps come out orders below the bound."""
    V1, ld, Tn, blank = 51866, 51968, 1500, 51865
    g = torch.Generator(device="cuda").manual_seed(9)
    buf = torch.randn(Tn, ld, device="cuda", generator=g).bfloat16().view(1, Tn, ld)
    buf[:, :, V1:] = NAN
    logits = buf[:, :, :V1]
    rng = np.random.default_rng(106)
    ys = [[int(t) for t in rng.integers(0, V1 - 1, 40)] for _ in range(2)]
    ys[1][7] = ys[1][6]                                                      # one repeat
    slices = [(0, 1500), (613, 375)]
    lse = torch.empty(Tn, device="cuda")
    L.call("dicow_ctc_frame_lse", logits.data_ptr(), 1, Tn, V1, ld, lse.data_ptr(), L.stream())
    al = pkg.ctc_forced_align(logits, ys, blank=blank, rows=[0, 0], frame_start=[s[0] for s in slices], frame_len=[s[1] for s in slices], lse=lse)
    al2 = pkg.ctc_forced_align(logits, ys, blank=blank, rows=[0, 0], frame_start=[s[0] for s in slices], frame_len=[s[1] for s in slices])
    assert torch.equal(al.path, al2.path) and torch.equal(al.score, al2.score)       # lse = None computes the same lse
    assert al.ok.tolist() == [True, True]
    for i, ((f0, F), y) in enumerate(zip(slices, ys)):
        cols = sorted(set(y)) + [blank]
        x32 = logits[0, f0:f0 + F][:, torch.tensor(cols, device="cuda")].float() - lse[f0:f0 + F, None]          # the kernel's own x
        x = x32.double().cpu().numpy()
        remap = {c: j for j, c in enumerate(cols)}
        want = R.align(x, [remap[t] for t in y], remap[blank])
        path = al.path[i, :F].cpu().tolist()
        R.check_path(path, y, blank)
        assert (al.path[i, F:] == -1).all()
        rescored = R.rescore(x, [remap[c] for c in path])
        bound = F * F * float(np.abs(x).max()) * 2.0 ** -24
        gap_score, gap_path = abs(float(al.score[i]) - want["score"]), want["score"] - rescored
        print(f"F={F} L=40: score {float(al.score[i]):.6f} best64 {want['score']:.6f} |score - best64| {gap_score:.3e} "
              f"best64 - rescored {gap_path:.3e} bound {bound:.3e}")
        assert want["status"] == 0 and gap_score < bound and -1e-9 <= gap_path < bound
        spans = al.spans[i, :40].cpu().tolist()
        assert all(path[s:e] == [t] * (e - s) and e > s for (s, e), t in zip(spans, y))
        tsum = float(al.token_score[i, :40].double().sum()) + sum(float(x[f, remap[blank]]) for f, c in enumerate(path) if c == blank)
        assert abs(tsum - rescored) < bound


def planted(paths, V1, seed, height=4.0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(len(paths), len(paths[0]), V1, generator=g) * 2.0 - 1.0).bfloat16().float()
    for b, p in enumerate(paths):
        x[b, torch.arange(len(p)), torch.tensor(p)] = height
    return x


def test_planted_spans_come_back_through_the_wrapper():
    """Logits with a known frame per token (4 above noise in [-1, 1]): exactly the planted spans, in seconds through token_timestamps;
    a list of lists and a padded tensor with lengths give the same; the 128-padded bf16 view is read in place."""
    V1, blank = 37, 36
    b = blank
    paths = [[b, b, 5, 5, b, 6, 7, 7, 7, b, 7, b], [9, 9, 9, b, b, b, 4, 4, 30, 30, 30, 30]]
    x = planted(paths, V1, 1)
    buf = torch.full((2, 12, 128), NAN, dtype=torch.bfloat16, device="cuda")
    buf[:, :, :V1] = x.cuda().bfloat16()
    logits = buf[:, :, :V1]
    ys = [[5, 6, 7, 7], [9, 4, 30]]
    al = pkg.ctc_forced_align(logits, ys, blank=blank)
    assert isinstance(al, pkg.CtcAlignment) and al.ok.tolist() == [True, True] and al.path.is_cuda and al.spans.dtype == torch.int32
    assert al.path.cpu().tolist() == paths
    assert al.spans.cpu().tolist() == [[[2, 4], [5, 6], [6, 9], [10, 11]], [[0, 3], [6, 8], [8, 12], [-1, -1]]]
    pad = torch.tensor([[5, 6, 7, 7], [9, 4, 30, 0]], device="cuda")
    al2 = pkg.ctc_forced_align(logits, pad, torch.tensor([4, 3]), blank=blank)
    assert all(torch.equal(a, c) for a, c in zip(al, al2))
    times = pkg.token_timestamps(al, 0.08, [10.0, 0.0])
    assert [t[0] for t in times[0]] == [5, 6, 7, 7] and [t[0] for t in times[1]] == [9, 4, 30]
    assert [t[1:3] for t in times[0]] == [pytest.approx((10.0 + 0.08 * s, 10.0 + 0.08 * e)) for s, e in ((2, 4), (5, 6), (6, 9), (10, 11))]
    lp = torch.log_softmax(logits.float(), -1).cpu()
    assert times[1][0][3] == pytest.approx(float(lp[1, 0:3, 9].mean()), abs=1e-5) and all(t[3] < 0 for t in times[0] + times[1])
    # a slice: frames 4 .. 11 of row 0 hold 6 7 7 (and the b between them), relative to frame_start
    al3 = pkg.ctc_forced_align(logits, [[6, 7, 7], [5] * 13, []], blank=blank, rows=[0, 0, 1], frame_start=[4, 0, 3], frame_len=[8, 12, 3])
    assert al3.ok.tolist() == [True, False, True] and al3.spans[0].cpu().tolist()[:3] == [[1, 2], [2, 5], [6, 7]]
    assert (al3.path[1] == -1).all() and (al3.spans[1] == -1).all() and float(al3.score[1]) == -np.inf
    assert al3.path[2].cpu().tolist() == [b, b, b] + [-1] * 9 and pkg.token_timestamps(al3, 0.02)[1:] == [None, []]
    with pytest.raises(L.DicowError, match="is the blank"):
        pkg.ctc_forced_align(logits, [[5, blank]], blank=blank)
    with pytest.raises(L.DicowError, match="past the T = 12"):
        pkg.ctc_forced_align(logits, [[5]], blank=blank, frame_start=[6], frame_len=[7])
    assert pkg.ctc_forced_align(logits, [], blank=blank).path.shape[0] == 0


def test_the_wrapper_splits_a_session_that_passes_the_workspace_limit(monkeypatch):
    V1, blank = 6, 0
    rng = np.random.default_rng(107)
    x = torch.from_numpy(dyadic(rng, (1, 50, V1))).float().cuda()
    ys = [targets(rng, int(rng.integers(0, 12)), V1, blank) for _ in range(9)]
    whole = pkg.ctc_forced_align(x, ys, blank=blank, rows=[0] * 9, normalized=True)
    from ts_asr_whisper_amd import ctc_align
    lib = L.lib()
    one = max(lib.dicow_ctc_align_ws_bytes(np.array([[0, 0, 50, 0, len(y)]], np.int64).ctypes.data, 1) for y in ys)
    real, calls = L.call, []

    class Small:
        """The library with a workspace limit of three problems."""

        def __getattr__(self, name):
            return getattr(lib, name)

        def dicow_ctc_align_ws_bytes(self, table, n):
            need = lib.dicow_ctc_align_ws_bytes(table, n)
            return -1 if need > 3 * one else need

    monkeypatch.setattr(L, "CTC_ALIGN_MAX_WS_BYTES", 3 * one)
    monkeypatch.setattr(L, "lib", lambda: Small())
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(a[10]) if name == "dicow_ctc_forced_align" else None, real(name, *a))[1])
    parts = ctc_align.ctc_forced_align(x, ys, blank=blank, rows=[0] * 9, normalized=True)
    assert len(calls) >= 3 and sum(calls) == 9
    assert all(torch.equal(a, c) for a, c in zip(whole, parts))


def test_align_segments_end_to_end():
    """The golden CTC model (2 s windows, 25 CTC frames of 80 ms each) on a two-window input: LongFormDecoder.transcribe's segments, one
    planted feasible segment and one that cannot fit its slice, through align_segments -> words_as_segments -> tcp_wer."""
    from ts_asr_whisper_amd.generation import LongFormDecoder
    from tests.test_gpu_model import build_model
    z = load_golden("f10_ctc")
    model, cfg = build_model(pkg, z, requires_grad=False)
    model.eval()
    ts0 = int(z["ts_start"])

    class Tok:
        prefix_tokens = [int(v) for v in z["prefix"]]
        upper_cased_tokens = {3: 13}
        all_special_ids = [cfg.eos_token_id]

        def get_vocab(self):
            v = {f"tok{i}": i for i in range(cfg.vocab_size)}
            for j in range(int(z["ts_n"])):
                v.pop(f"tok{ts0 + j}")
                v[f"<|{0.02 * j:.2f}|>"] = ts0 + j
            return v

        def decode(self, ids):
            return "".join((" w%d" if i % 3 else "x%d") % i for i in ids)

    model.set_tokenizer(Tok())
    W = 2 * cfg.max_source_positions
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(2, cfg.num_mel_bins, 2 * W, generator=g).clamp_(-1.5, 1.5).cuda()
    stno = torch.softmax(torch.randn(2, 4, W, generator=g) * 2, 1).cuda()
    prompt = torch.tensor([[cfg.decoder_start_token_id, 7]])
    segs = LongFormDecoder(model).transcribe(feats, stno, [2 * W, 2 * W], prompt, ts0 - 1, eos_token_id=5, pad_token_id=cfg.pad_token_id,
                                             max_new_tokens=8)
    n_decoded = [len(s) for s in segs]
    segs[0].append(dict(start=0.5, end=1.5, tokens=[ts0 + 25, 21, 22, 13, 24, ts0 + 75]))
    segs[1].append(dict(start=3.0, end=3.1, tokens=[20] * 30))
    Tn, _ = model.get_encoder().ctc_logits_layout()
    fs, margin, total = 0.01 * W / Tn, 0.16, 0.01 * 2 * W
    out = pkg.align_segments(model, feats, stno, segs, margin_s=margin)
    assert [len(s) for s in out] == [n + 1 for n in n_decoded] and all("words" not in s for r in segs for s in r)
    for r in out:
        for s in r:
            assert s["aligned"] in (True, False) and isinstance(s["words"], list)
            lo, hi = max(s["start"] - margin - fs, 0.0), min(s["end"] + margin + fs, total)
            times = [(w[1], w[2]) for w in s["words"]]
            assert all(a <= b for a, b in times) and all(times[k][1] <= times[k + 1][0] + 1e-9 for k in range(len(times) - 1))
            if s["aligned"]:
                assert all(lo - 1e-9 <= a and b <= hi + 1e-9 for a, b in times), (s, lo, hi)
                assert all(0.0 < w[3] <= 1.0 for w in s["words"])
    mine, bad = out[0][-1], out[1][-1]
    assert mine["aligned"] and [w[0] for w in mine["words"]] == ["x21", "w22", "w13x24"]
    assert not bad["aligned"] and [w[0] for w in bad["words"]] == ["w20"] * 30 and bad["words"][0][3] is None
    assert bad["words"][0][1] == 3.0 and bad["words"][-1][2] == pytest.approx(3.1) and len({round(w[2] - w[1], 9) for w in bad["words"]}) <= 2
    hyp = pkg.words_as_segments(out[0], "A")
    assert len(hyp) == sum(len(s["words"]) for s in out[0]) and all(isinstance(h["words"], str) and " " not in h["words"] for h in hyp)
    res = pkg.tcp_wer([("A", 0.4, 1.6, "x21 w22 w13x24")], [h for h in hyp if h["start_time"] >= 0.0][-3:], collar=0.1)
    assert isinstance(res, dict)
    model.config.ctc_weight = 0.0
    with pytest.raises(L.DicowError, match="ctc_weight"):
        pkg.align_segments(model, feats, stno, segs)
