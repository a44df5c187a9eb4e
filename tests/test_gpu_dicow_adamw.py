"""``DiCoWAdamW`` / ``clip_grad_norm_`` (ts-asr-whisper_amd/optim.py, csrc/optim.hip) against torch's own AdamW and clip on the same GPU.
Run with `pytest -m gpu`.

The parity bound.  The kernel evaluates torch's single-tensor AdamW expression by expression with the same fp32 scalars, so per step
the two differ only where the compilers contract a multiply-add differently: a few fp32 roundings of the update u = step_size m /
denom (|u| <= lr * (1 - beta1) / sqrt(1 - beta2) ~ 3.2 lr), i.e. |du| < 1e-6 lr, plus at most one rounding of p itself (1 ulp).
Over k steps these add up (m and v carry theirs forward the same way), so we require
    |p - p_torch| <= k * (2 ulp(p_torch) + 1e-4 lr)
-- a hundredfold margin on the lr term.  Each test also runs the WRONG variants with torch and checks that the bound rejects them by
at least 100x: weight decay applied to the wd-0 group (lr wd |p| per step = 5e-4 |p|), a group-wide step count instead of the
per-parameter one (bias correction of step 4 instead of 1: the first update 3.4x too small), the scheduler's lr ignored (up to half
the lr per step) and, with max_grad_norm, a missing clip coefficient (eps = 1e-3 makes the update depend on the gradient scale)."""
import copy
import io
import math

import pytest
import torch

import amd_pkg

pytestmark = pytest.mark.gpu
pkg = amd_pkg.load()
from ts_asr_whisper_amd import _lib as L  # noqa: E402
from ts_asr_whisper_amd.optim import DiCoWAdamW, clip_grad_norm_  # noqa: E402

SIZES = [1, 3, 5, 1280, 1281, 4097, 1280 * 5120, 6_553_607, 7, 64, 1279, 16384, 16385, 50_000, 2, 1280 * 4, 333, 4096, 17, 1024 * 9 + 1]
LR1, LR2 = 1e-3, 1e-2


def _ulp(x):
    a = x.abs()
    return torch.nextafter(a, torch.full_like(a, math.inf)) - a


def _excess(p, q, lr, steps):
    """max of |p - q| / bound (<= 1: within the bound)."""
    p, q = p.detach(), q.detach()
    b = steps * (2 * _ulp(q) + 1e-4 * lr)
    return float(((p - q).abs() / b).max())


def _params(seed=0):
    """~40 fp32 tensors over two groups: group 0 (lr 1e-3, wd 0.05) and group 1 (lr 1e-2, wd 0); the LAST parameter of group 1 is an
    offset view into a larger storage (4 bytes off: scalar path), index `late` of group 1 gets no gradient for the first 3 steps."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    vals = [torch.randn(n, device="cuda", generator=g) * 0.1 for n in SIZES + SIZES]
    return vals


def _make(vals, offset_view=True):
    ps = [torch.nn.Parameter(v.clone()) for v in vals]
    if offset_view:
        big = torch.zeros(vals[-1].numel() + 9, device="cuda")
        big[1:1 + vals[-1].numel()] = vals[-1]
        ps[-1] = torch.nn.Parameter(big[1:1 + vals[-1].numel()])
        assert ps[-1].data_ptr() % 16 == 4 and ps[-1].storage_offset() == 1
    h = len(ps) // 2
    return ps, [{"params": ps[:h], "lr": LR1, "weight_decay": 0.05}, {"params": ps[h:], "lr": LR2, "weight_decay": 0.0}]


LATE = -3          # (index into the parameter list) no gradient before step 4


def _grads(step, vals, seed=100, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed + step)
    return [torch.randn(v.numel(), device="cuda", generator=g) * scale for v in vals]


def _cos(k, total=10):
    return 0.5 * (1.0 + math.cos(math.pi * k / total))


def _run(kind, vals, steps=10, sched=True, late_zero=False, wd2=0.0, max_grad_norm=None, clip_first=False, eps=1e-8, scale=1.0,
         offset_view=True):
    ps, groups = _make(vals, offset_view)
    groups[1]["weight_decay"] = wd2
    if kind == "torch":
        opt = torch.optim.AdamW(groups, eps=eps, foreach=False)
    else:
        opt = DiCoWAdamW(groups, eps=eps, max_grad_norm=max_grad_norm)
    lam = torch.optim.lr_scheduler.LambdaLR(opt, _cos) if sched else None
    for s in range(steps):
        gs = _grads(s, vals, scale=scale)
        for i, (p, g) in enumerate(zip(ps, gs)):
            p.grad = g.view_as(p)
        if s < 3:
            ps[LATE].grad = torch.zeros_like(ps[LATE]) if late_zero else None
        if clip_first:
            (torch.nn.utils.clip_grad_norm_ if kind == "torch" else clip_grad_norm_)(ps, 1.0)
        opt.step()
        if lam is not None:
            lam.step()
    torch.cuda.synchronize()
    return ps, opt


def _worst(ps, ref, steps=10):
    h = len(ps) // 2
    return max(_excess(p, q, LR1 if i < h else LR2, steps) for i, (p, q) in enumerate(zip(ps, ref)))


@pytest.fixture(scope="module")
def vals():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _params()


def test_parity_with_torch_adamw_two_groups_schedule_late_param(vals):
    ref, _ = _run("torch", vals)
    ours, opt = _run("dicow", vals)
    assert _worst(ours, ref) <= 1.0
    h = len(ref) // 2
    assert float(opt.state[ours[LATE]]["step"]) == 7.0 and float(opt.state[ours[0]]["step"]) == 10.0   # per-parameter step counts
    # the bound rejects each wrong variant by at least 100x
    wrong_wd, _ = _run("torch", vals, wd2=0.05)
    assert max(_excess(p, q, LR2, 10) for p, q in zip(wrong_wd[h:], ref[h:])) > 100
    wrong_step, _ = _run("torch", vals, late_zero=True)
    assert _excess(wrong_step[LATE], ref[LATE], LR2, 10) > 100
    wrong_lr, _ = _run("torch", vals, sched=False)
    assert _worst(wrong_lr, ref) > 100


def test_bit_reproducible(vals):
    a, oa = _run("dicow", vals, steps=4, max_grad_norm=1.0)
    b, ob = _run("dicow", vals, steps=4, max_grad_norm=1.0)
    for p, q in zip(a, b):
        assert torch.equal(p, q)
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(oa.state[p][k], ob.state[q][k])
    assert torch.equal(oa.last_grad_norm, ob.last_grad_norm)


def test_step_refreshes_the_models_bf16_weights():
    """One forward/backward and one DiCoWAdamW step; the next forward equals, bit for bit, a fresh twin loaded with the updated
    state dict (a missing version bump leaves the model on its stale bf16 weight copies)."""
    from tests.test_gpu_hf_trainer import _cfg, _build, _samples, _collate
    cfg = _cfg(pkg)
    items = _samples(cfg, 2)
    batch = {k: v.cuda() for k, v in _collate(items).items()}
    model = _build(pkg, cfg).cuda()
    opt = pkg.dicow_optimizer(model, 1e-3)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        model(**batch).loss.backward()
    opt.step()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        after = model(**batch).logits.float()
    twin = _build(pkg, cfg)
    twin.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    twin = twin.cuda()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        fresh = twin(**batch).logits.float()
    assert torch.equal(after, fresh)


def _steps(opt, ps, vals, lo, hi):
    for s in range(lo, hi):
        for p, g in zip(ps, _grads(s, vals)):
            p.grad = g.view_as(p)
        opt.step()
    torch.cuda.synchronize()


def test_state_dict_resume_is_bit_equal_and_cross_loads_with_torch(vals):
    ps, groups = _make(vals)
    full = DiCoWAdamW(groups)
    _steps(full, ps, vals, 0, 4)
    # stop after 2, save with torch.save, load into a fresh optimizer, 2 more
    qs, groups = _make(vals)
    half = DiCoWAdamW(groups)
    _steps(half, qs, vals, 0, 2)
    buf = io.BytesIO()
    torch.save(half.state_dict(), buf)
    rs, groups = _make([q.detach() for q in qs])
    again = DiCoWAdamW(groups)
    again.load_state_dict(torch.load(io.BytesIO(buf.getvalue())))
    _steps(again, rs, vals, 2, 4)
    for a, b in zip(ps, rs):
        assert torch.equal(a, b)
    # torch -> DiCoWAdamW and DiCoWAdamW -> torch: same keys / shapes, continuation within the bound
    for src_cls, dst_cls in ((torch.optim.AdamW, DiCoWAdamW), (DiCoWAdamW, torch.optim.AdamW)):
        ps, groups = _make(vals)
        src = src_cls(groups, **({"foreach": False} if src_cls is torch.optim.AdamW else {}))
        _steps(src, ps, vals, 0, 2)
        sd = copy.deepcopy(src.state_dict())                           # (state_dict() shares the live step tensors)
        qs, groups = _make([p.detach() for p in ps])
        dst = dst_cls(groups, **({"foreach": False} if dst_cls is torch.optim.AdamW else {}))
        dst.load_state_dict(sd)
        assert sd["param_groups"][0].keys() == dst.state_dict()["param_groups"][0].keys()
        _steps(src, ps, vals, 2, 4)
        _steps(dst, qs, vals, 2, 4)
        dsd = dst.state_dict()
        for i, st in sd["state"].items():
            assert set(st) == set(dsd["state"][i]) == {"step", "exp_avg", "exp_avg_sq"}
            assert dsd["state"][i]["step"].device.type == "cpu" and float(dsd["state"][i]["step"]) == 4.0
            assert st["exp_avg"].shape == dsd["state"][i]["exp_avg"].shape
        assert _worst(qs, ps, 4) <= 1.0


def test_clip_grad_norm_against_torch_inf_repeat_and_fused(vals):
    gs = _grads(0, vals, scale=3.0)
    mine = [torch.nn.Parameter(torch.zeros_like(g)) for g in gs]
    theirs = [torch.nn.Parameter(torch.zeros_like(g)) for g in gs]
    for p, q, g in zip(mine, theirs, gs):
        p.grad, q.grad = g.clone(), g.clone()
    n_t = torch.nn.utils.clip_grad_norm_(theirs, 1.0)
    n_m = clip_grad_norm_(mine, 1.0)
    assert n_m.dim() == 0 and n_m.is_cuda
    assert abs(float(n_m) - float(n_t)) <= 1e-5 * float(n_t)
    coef = torch.clamp(1.0 / (n_m + 1e-6), max=1.0)                       # torch's formula on OUR norm: the scaling itself is exact
    for p, q, g in zip(mine, theirs, gs):
        assert bool(((p.grad - g * coef).abs() <= 2 * _ulp(g * coef)).all())
        assert bool(((p.grad - q.grad).abs() <= 1e-5 * q.grad.abs() + 1e-30).all())
    # max_norm = inf: the norm only, gradients bit-unchanged
    for p, g in zip(mine, gs):
        p.grad = g.clone()
    n_inf = clip_grad_norm_(mine, math.inf)
    assert torch.equal(n_inf, n_m) and all(torch.equal(p.grad, g) for p, g in zip(mine, gs))
    # repeated calls are bit-identical
    again = clip_grad_norm_(mine, 1.0)
    first = [p.grad.clone() for p in mine]
    for p, g in zip(mine, gs):
        p.grad = g.clone()
    assert torch.equal(clip_grad_norm_(mine, 1.0), again) and all(torch.equal(p.grad, f) for p, f in zip(mine, first))
    # fused clip == clip_grad_norm_ + DiCoWAdamW (within the bound), p.grad left unscaled; torch with the clip is the reference
    kw = dict(steps=4, eps=1e-3, scale=3.0)
    fused, of = _run("dicow", vals, max_grad_norm=1.0, **kw)
    split, _ = _run("dicow", vals, clip_first=True, **kw)
    ref, _ = _run("torch", vals, clip_first=True, **kw)
    assert _worst(fused, split, 4) <= 1.0 and _worst(fused, ref, 4) <= 1.0
    last = _grads(3, vals, scale=3.0)
    assert all(torch.equal(p.grad.reshape(-1), g) for p, g in zip(fused, last) if p.grad is not None)
    assert abs(float(of.last_grad_norm) - float(torch.cat(last).norm())) <= 1e-5 * float(of.last_grad_norm)
    unclipped, _ = _run("torch", vals, **kw)                               # the wrong variant: the clip coefficient missing
    assert _worst(unclipped, ref, 4) > 100


def test_headline_parameter_list_one_step():
    """743 tensors / 637,296,640 elements (whisper-large-v3-turbo, decoder frozen, shapes from the meta-device model) in the
    reference's two groups: one step against torch.optim.AdamW within the bound (int64 offsets, the table at full size; ~20 GB)."""
    from ts_asr_whisper_amd.trainer import freeze_by_keyword
    cfg = pkg.DiCoWConfig.preset("whisper-large-v3-turbo")
    with torch.device("meta"):
        meta = pkg.DiCoWForConditionalGeneration(cfg)
    freeze_by_keyword(meta, ("decoder",))
    pre = ("model.encoder.fddts", "model.encoder.initial_fddt")
    named = [(n, p.shape) for n, p in meta.named_parameters() if p.requires_grad]
    assert len(named) == 743 and sum(math.prod(s) for _, s in named) == 637_296_640
    gen = torch.Generator(device="cuda").manual_seed(5)
    mk = lambda: [torch.nn.Parameter(torch.empty(s, device="cuda")) for _, s in named]
    ours, theirs = mk(), mk()
    for p, q in zip(ours, theirs):
        p.data.normal_(0, 0.02, generator=gen)
        q.data.copy_(p.data)
        p.grad = torch.randn(p.shape, device="cuda", generator=gen)
        q.grad = p.grad.clone()
    split = lambda ps: [{"params": [p for (n, _), p in zip(named, ps) if not n.startswith(pre)]},
                        {"params": [p for (n, _), p in zip(named, ps) if n.startswith(pre)], "lr": 2e-2, "weight_decay": 0.0}]
    DiCoWAdamW(split(ours), lr=2e-4, weight_decay=0.01).step()
    torch.optim.AdamW(split(theirs), lr=2e-4, weight_decay=0.01, foreach=False).step()
    torch.cuda.synchronize()
    worst = max(_excess(p, q, 2e-2 if n.startswith(pre) else 2e-4, 1) for (n, _), p, q in zip(named, ours, theirs))
    assert worst <= 1.0


def test_errors():
    p = torch.nn.Parameter(torch.zeros(8, device="cuda"))
    with pytest.raises(NotImplementedError):
        DiCoWAdamW([p], amsgrad=True)
    with pytest.raises(NotImplementedError):
        DiCoWAdamW([p], lr=torch.tensor(1e-3))
    b = torch.nn.Parameter(torch.zeros(8, device="cuda", dtype=torch.bfloat16))
    b.grad = torch.ones_like(b)
    with pytest.raises(L.DicowError, match="float32"):
        DiCoWAdamW([b]).step()
    s = torch.nn.Parameter(torch.zeros(8, 4, device="cuda"))
    s.grad = torch.eye(8, 4, device="cuda").to_sparse()
    with pytest.raises(L.DicowError, match="sparse"):
        DiCoWAdamW([s]).step()
    c = torch.nn.Parameter(torch.zeros(8))
    c.grad = torch.ones(8)
    with pytest.raises(L.DicowError, match="GPU"):
        DiCoWAdamW([c]).step()
