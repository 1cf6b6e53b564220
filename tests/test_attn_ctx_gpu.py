"""Limited-context relative-position attention (NeMo att_context_size / att_context_style): the windowed
kernels kdfm_relpos_attn_ctx_fwd / kdfm_relpos_attn_ctx_bwd (bf16 MFMA, csrc/attn_fused.hip and attn_bwd.hip
CTX instantiations) and kdfm_relpos_softmax_ctx_fwd (the f32 parity route).

The float64 reference is test_attn_bwd_gpu.py's `_torch_grads` with the window added to the key mask, the
window in the per-query interval form of the reference's `_create_masks` (conformer_encoder.py:796-850):
query i sees keys [lo(i), hi(i)] intersected with the valid frames,
  regular (L, R):          lo = i - L (0 when L = -1), hi = i + R (T-1 when R = -1);
  chunked_limited (L, R):  chunk = R + 1, c = i // chunk, lo = (c - L // chunk) chunk, hi = (c + 1) chunk - 1.

Tolerances are the project's for these bf16 kernels: O within 1e-2 of max |O| (test_attn_fused_gpu.py), lse
within 2e-2 max(1, |lse|) and every gradient within 2e-2 relative Frobenius error (test_attn_bwd_gpu.py);
against the unfused f32 chain with attention dropout 0.1 the same 2e-2.  The f32 softmax is compared with
float64 at 1e-5 absolute (P <= 1; __expf of an argument of magnitude <= ~20 is good to ~1e-6 relative and a
row sums <= 201 terms -- ten times that; the 2e-3 of test_attn_fused_gpu.py is a bf16-operand bound)."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(3, 2, 201, 88), (2, 8, 201, 512), (2, 8, 130, 1024), (3, 2, 77, 88)]   # head dims 44, 64, 128
REGULAR = [(0, 0), (1, 0), (40, 20), (64, 63), (63, 64), (-1, 0), (16, -1)]
CHUNKED = [(48, 15), (128, 31)]
WINDOWS = [(w, "regular") for w in REGULAR] + [(w, "chunked_limited") for w in CHUNKED]
GNAMES = ("dQu", "dQv", "dK", "dV", "dPpos")


def _rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _lens(B, T):
    """test_attn_bwd_gpu.py's ragged lengths; the three-utterance shapes end with an utterance of length 1
    (T = 201) or one shorter than the 16..128-frame windows (13 frames, T = 77), the 130-frame shape's
    second utterance has 13 frames too."""
    lens = [T] + [max(1, T - 23 * (i + 1)) for i in range(B - 1)]
    if B == 3:
        lens[2] = 1 if T == 201 else 13
    if T == 130:
        lens[1] = 13
    return lens


@functools.lru_cache(maxsize=None)
def _inputs(B, H, T, d):
    g = torch.Generator(device="cuda").manual_seed(T + d)
    rows = B * T
    qkv = torch.randn(rows, 3 * d, device="cuda", generator=g)
    qu = torch.randn(rows, d, device="cuda", generator=g)
    qv = torch.randn(rows, d, device="cuda", generator=g)
    ppos = torch.randn(2 * T - 1, d, device="cuda", generator=g)
    do = torch.randn(rows, d, device="cuda", generator=g)
    lens = torch.tensor(_lens(B, T), dtype=torch.int64, device="cuda")
    return qkv, qu, qv, ppos, do, lens


def _triple(size, style):
    from kdfm.config import att_context_triple
    return att_context_triple(size, style)


def _window(T, size, style):
    """(T, T) bool, True = visible: the interval form of the module docstring."""
    L, R = size
    i = torch.arange(T, device="cuda")
    if style == "chunked_limited" and R >= 0:
        chunk = R + 1
        c = i // chunk
        lo = torch.zeros_like(i) if L < 0 else (c - L // chunk) * chunk
        hi = (c + 1) * chunk - 1
    else:
        lo = torch.zeros_like(i) if L < 0 else i - L
        hi = torch.full_like(i, T - 1) if R < 0 else i + R
    j = i[None, :]
    return (j >= lo[:, None]) & (j <= hi[:, None])


@functools.lru_cache(maxsize=None)
def _reference(B, H, T, d, size, style):
    """float64 autograd with the banded mask: O, lse, the norms of the uncancelled score-side gradients and the
    five gradients (computed once per case)."""
    qkv, qu, qv, ppos, do, lens = _inputs(B, H, T, d)
    dk = d // H
    f = lambda t: t.double().detach().clone().requires_grad_(True)  # noqa: E731
    q_u, q_v, k, v, pp = f(qu), f(qv), f(qkv[:, d:2 * d]), f(qkv[:, 2 * d:]), f(ppos)
    sh = lambda t: t.view(B, T, H, dk).permute(0, 2, 1, 3)  # noqa: E731
    ac = sh(q_u) @ sh(k).transpose(-1, -2)
    bdf = torch.einsum("bhic,hrc->bhir", sh(q_v), pp.view(2 * T - 1, H, dk).permute(1, 0, 2))
    idx = (T - 1 - torch.arange(T, device="cuda")[:, None] + torch.arange(T, device="cuda")[None, :])
    bd = torch.gather(bdf, 3, idx.expand(B, H, T, T))
    s = (ac + bd) / math.sqrt(dk)
    keym = torch.arange(T, device="cuda")[None, :] < lens[:, None]
    vis = keym[:, None, None, :] & _window(T, size, style)[None, None]
    s = s.masked_fill(~vis, float("-inf"))
    lse = torch.logsumexp(s, -1).detach()
    P = torch.softmax(s, -1)
    P = torch.where(keym[:, None, :, None], P, torch.zeros_like(P))
    O = (P @ sh(v)).permute(0, 2, 1, 3).reshape(B * T, d)
    loss = (O * do.double()).sum()
    grads = torch.autograd.grad(loss, [q_u, q_v, k, v, pp], retain_graph=True)
    # the score-side gradients BEFORE the softmax cancellation dS = P (dP - r): the same linear maps applied to
    # P |dP| scale (test_ctx_forward_backward_match_float64's zero-reference case)
    dP = sh(do.double()) @ sh(v).detach().transpose(-1, -2)
    W = (P * dP.abs()).detach()
    s_fin = torch.where(vis, s, torch.zeros_like(s))
    unc = torch.autograd.grad((s_fin * W).sum(), [q_u, q_v, k, pp])
    return O.detach(), lse, tuple(u.norm().item() for u in unc), grads


def _ctx_run(K, B, H, T, d, p, seed, ctx, poison=False):
    """windowed forward (O, lse) then the windowed backward; returns (O, lse, dQu, dQv, dK, dV, dPpos, dS, Pd)."""
    qkv, qu, qv, ppos, do, lens = _inputs(B, H, T, d)
    sc = 1.0 / math.sqrt(d // H)
    fill = float("nan") if poison else 0.0
    o = torch.full((B * T, d), fill, device="cuda")
    lse = torch.full((B, H, T), fill, device="cuda")
    K.relpos_attn_ctx_fwd(qu, qv, qkv, ppos, lens, o, B, H, T, sc, p, seed, 11, ctx, lse=lse)
    dqu = torch.full((B * T, d), fill, device="cuda")
    dqv = torch.full((B * T, d), fill, device="cuda")
    dqkv = torch.full((B * T, 3 * d), fill, device="cuda")
    dpos = torch.full((2 * T - 1, d), fill, device="cuda")
    dS, Pd = K.attn_bwd2_saved(B, H, T, "cuda")
    ws = torch.full((K.relpos_attn_bwd2_dpos_ws(B, T, d),), fill, device="cuda")
    if poison:
        dS.fill_(float("nan"))
        Pd.fill_(float("nan"))
    K.relpos_attn_ctx_bwd(do, o, qu, qv, qkv, ppos, lse, lens, dqu, dqv, dqkv, dpos, B, H, T, sc, p, seed, 11, ctx,
                          ds=dS, pd=Pd, ws=ws)
    torch.cuda.synchronize()
    return o, lse, dqu, dqv, dqkv[:, d:2 * d], dqkv[:, 2 * d:], dpos, dS, Pd


@pytest.mark.parametrize("size", [(-1, -1), (500, 500)])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_non_binding_window_is_bitwise_full_context(size, p):
    """A window that covers every key: O, lse and all five gradients are bitwise those of relpos_attn_fwd +
    relpos_attn_bwd2_dq / _dkv / _dpos (T = 77)."""
    from kdfm import kernels as K
    B, H, T, d = 3, 2, 77, 88
    qkv, qu, qv, ppos, do, lens = _inputs(B, H, T, d)
    seed = torch.tensor([4243], dtype=torch.int64, device="cuda")
    sc = 1.0 / math.sqrt(d // H)
    lse = torch.empty(B, H, T, device="cuda")
    o = torch.empty(B * T, d, device="cuda")
    K.relpos_attn_fwd(qu, qv, qkv, ppos, lens, o, None, None, B, H, T, sc, p, seed, 11, lse=lse)
    dqu = torch.empty(B * T, d, device="cuda")
    dqv = torch.empty_like(dqu)
    dqkv = torch.zeros(B * T, 3 * d, device="cuda")
    dpos = torch.empty(2 * T - 1, d, device="cuda")
    dS, Pd = K.attn_bwd2_saved(B, H, T, "cuda")
    K.relpos_attn_bwd2_dq(do, o, qu, qv, qkv, ppos, lse, lens, None, dS, Pd, dqu, dqv, B, H, T, sc, p, seed, 11)
    K.relpos_attn_bwd2_dpos(qv, dS, lens, dpos, B, H, T)
    K.relpos_attn_bwd2_dkv(do, qu, dS, Pd, lens, dqkv, B, H, T)
    torch.cuda.synchronize()
    want = (o, lse, dqu, dqv, dqkv[:, d:2 * d], dqkv[:, 2 * d:], dpos)
    got = _ctx_run(K, B, H, T, d, p, seed, _triple(size, "regular"))
    for name, a, b in zip(("O", "lse") + GNAMES, got, want):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("B,H,T,d", SHAPES)
@pytest.mark.parametrize("size,style", WINDOWS)
def test_ctx_forward_backward_match_float64(B, H, T, d, size, style):
    """No dropout, against float64 autograd with the banded mask.  Forward: O within 1e-2 of max |O|, padded
    query rows exactly zero, lse (of the centred keys' scores, attn_centre.h) within 2e-2 max(1, |lse|), 3e38
    on padded rows.  Backward: rel. Frobenius <= 2e-2 for dQu, dQv, dK, dV, dPpos; keys past a length get
    exactly zero dK / dV; for regular windows the dPpos rows of relative positions i - j outside [-R, L] are
    exactly zero.

    Window (0, 0): every query sees one key, P = 1 and dS = P (dP - r) is exactly zero, so the float64 dQu, dQv,
    dK and dPpos are zero (1e-16 of roundoff) and an error relative to them is undefined (measured: 2e29 .. 8e29
    on the four shapes).  Where the reference norm is below 1e-6 of the norm BEFORE that cancellation -- the
    same linear maps applied to P |dP| scale, the quantity whose bf16 rounding (2^-9 relative) the kernels' dS
    error consists of -- the 2e-2 bounds the error relative to that uncancelled norm instead.  Every other
    window, (1, 0) included, meets 2e-2 against its own reference (measured <= 6.1e-3)."""
    from kdfm import kernels as K
    from test_attn_fused_gpu import kv_centred
    qkv, qu, qv, ppos, do, lens = _inputs(B, H, T, d)
    o_ref, lse_ref, unc, ref = _reference(B, H, T, d, size, style)
    o, lse, *got = _ctx_run(K, B, H, T, d, 0.0, None, _triple(size, style))[:7]
    err = (o.double() - o_ref).abs().max().item()
    print(f"O max err {err:.3e} of max |O| {o_ref.abs().max().item():.3e}")
    assert err <= 1e-2 * o_ref.abs().max().item(), err
    kc = (qkv - kv_centred(qkv, lens, B, T, d))[:, d:2 * d].double().view(B, T, H, d // H)
    shift = (qu.double().view(B, T, H, d // H) * kc).sum(-1).permute(0, 2, 1) / math.sqrt(d // H)
    want = lse_ref - shift
    for bi in range(B):
        L = int(lens[bi])
        lerr = (lse[bi, :, :L].double() - want[bi, :, :L]).abs().max().item()
        assert lerr <= 2e-2 * max(1.0, want[bi, :, :L].abs().max().item()), (bi, lerr)
        if L < T:
            assert (lse[bi, :, L:] == 3.0e38).all()
            assert o.view(B, T, d)[bi, L:].abs().max().item() == 0.0
    uncn = dict(zip(("dQu", "dQv", "dK", "dPpos"), unc))
    errs = {}
    for n, a, w in zip(GNAMES, got, ref):
        if n in uncn and w.norm().item() < 1e-6 * uncn[n]:   # zero reference: relative to the uncancelled norm
            errs[n] = (a.double() - w).norm().item() / uncn[n]
        else:
            errs[n] = _rel(a, w)
    print("rel. Frobenius", {n: f"{e:.3e}" for n, e in errs.items()})
    for n, e in errs.items():
        assert e <= 2e-2, (n, e)
    dk_, dv_, dpos = got[2], got[3], got[4]
    for bi in range(B):
        L = int(lens[bi])
        if L < T:
            assert dk_.view(B, T, d)[bi, L:].abs().max().item() == 0.0
            assert dv_.view(B, T, d)[bi, L:].abs().max().item() == 0.0
    if style == "regular":
        Lc, Rc = size
        rel = T - 1 - torch.arange(2 * T - 1, device="cuda")   # i - j of position row r
        outside = torch.zeros_like(rel, dtype=torch.bool)
        if Lc >= 0:
            outside |= rel > Lc
        if Rc >= 0:
            outside |= rel < -Rc
        if outside.any():
            assert dpos[outside].abs().max().item() == 0.0


def _unfused_ctx(K, B, H, T, d, p, seed, ctx):
    """test_attn_bwd_gpu.py's unfused f32 chain over relpos_softmax_ctx_fwd's P / P_drop (the f32 parity
    route of the encoder, same counter-RNG dropout mask): returns (O, (dQu, dQv, dK, dV, dPpos))."""
    from kdfm import _lib
    qkv, qu, qv, ppos, do, lens = _inputs(B, H, T, d)
    dk = d // H
    npos = 2 * T - 1
    sc = 1.0 / math.sqrt(dk)
    f32 = dict(math="f32")
    ac = torch.empty(B, H, T, T, device="cuda")
    K.gemm(qu, qkv[:, d:], ac, T, T, dk, d, 1, 1, 3 * d, T, 1, amode=_lib.LD_KC, bmode=_lib.LD_KC,
           batch=(B, H), bA=(T * d, dk), bB=(T * 3 * d, dk), bC=(H * T * T, T * T), **f32)
    bd = torch.empty(B, H, T, npos, device="cuda")
    K.gemm(qv, ppos, bd, T, npos, dk, d, 1, 1, d, npos, 1, amode=_lib.LD_KC, bmode=_lib.LD_KC,
           batch=(B, H), bA=(T * d, dk), bB=(0, dk), bC=(H * T * npos, T * npos), **f32)
    P = torch.empty(B, H, T, T, device="cuda")
    Pd = torch.empty_like(P)
    K.relpos_softmax_ctx_fwd(ac, bd, lens, P, Pd, B, H, T, sc, p, seed, 11, ctx)
    o = torch.empty(B * T, d, device="cuda")
    K.gemm(Pd, qkv[:, 2 * d:], o, T, dk, T, T, 1, 3 * d, 1, d, 1, amode=_lib.LD_KC, bmode=_lib.LD_XC,
           batch=(B, H), bA=(H * T * T, T * T), bB=(T * 3 * d, dk), bC=(T * d, dk), **f32)
    dPd = torch.empty(B, H, T, T, device="cuda")
    K.gemm(do, qkv[:, 2 * d:], dPd, T, T, dk, d, 1, 1, 3 * d, T, 1, amode=_lib.LD_KC, bmode=_lib.LD_KC,
           batch=(B, H), bA=(T * d, dk), bB=(T * 3 * d, dk), bC=(H * T * T, T * T), **f32)
    dac = torch.empty(B, H, T, T, device="cuda")
    dbd = torch.empty(B, H, T, npos, device="cuda")
    K.relpos_softmax_bwd(P, dPd, dac, dbd, B, H, T, sc, p, seed, 11)
    rows = B * T
    r_dv = torch.zeros(rows, d, device="cuda")
    K.gemm(Pd, do, r_dv, T, dk, T, 1, T, d, 1, d, 1, amode=_lib.LD_XC, bmode=_lib.LD_XC,
           batch=(B, H), bA=(H * T * T, T * T), bB=(T * d, dk), bC=(T * d, dk), **f32)
    r_dqu = torch.zeros(rows, d, device="cuda")
    K.gemm(dac, qkv[:, d:], r_dqu, T, dk, T, T, 1, 3 * d, 1, d, 1, amode=_lib.LD_KC, bmode=_lib.LD_XC,
           batch=(B, H), bA=(H * T * T, T * T), bB=(T * 3 * d, dk), bC=(T * d, dk), **f32)
    r_dk = torch.zeros(rows, d, device="cuda")
    K.gemm(dac, qu, r_dk, T, dk, T, 1, T, d, 1, d, 1, amode=_lib.LD_XC, bmode=_lib.LD_XC,
           batch=(B, H), bA=(H * T * T, T * T), bB=(T * d, dk), bC=(T * d, dk), **f32)
    r_dqv = torch.zeros(rows, d, device="cuda")
    K.gemm(dbd, ppos, r_dqv, T, dk, npos, npos, 1, d, 1, d, 1, amode=_lib.LD_KC, bmode=_lib.LD_XC,
           batch=(B, H), bA=(H * T * npos, T * npos), bB=(0, dk), bC=(T * d, dk), **f32)
    r_dpos = torch.zeros(npos, d, device="cuda")
    K.gemm(dbd, qv, r_dpos, npos, dk, T, 1, npos, d, 1, d, 1, amode=_lib.LD_XC, bmode=_lib.LD_XC,
           batch=(B, H), bA=(H * T * npos, T * npos), bB=(T * d, dk), bC=(0, dk), epi=_lib.EPI_ATOMIC, **f32)
    torch.cuda.synchronize()
    return o, (r_dqu, r_dqv, r_dk, r_dv, r_dpos)


@pytest.mark.parametrize("B,H,T,d", SHAPES)
@pytest.mark.parametrize("size,style", [((40, 20), "regular"), ((-1, 0), "regular"), ((48, 15), "chunked_limited")])
def test_ctx_matches_unfused_with_dropout(B, H, T, d, size, style):
    """Attention dropout 0.1: the windowed fused kernels against the unfused f32 chain over
    relpos_softmax_ctx_fwd's P / P_drop (same counter-RNG mask): O within 1e-2 and every gradient within 2e-2
    relative Frobenius error, as test_attn_bwd_gpu.py::test_attn_bwd_matches_unfused_with_dropout."""
    from kdfm import kernels as K
    p = 0.1
    seed = torch.tensor([4242], dtype=torch.int64, device="cuda")
    ctx = _triple(size, style)
    o, _, *got = _ctx_run(K, B, H, T, d, p, seed, ctx)[:7]
    o_ref, ref = _unfused_ctx(K, B, H, T, d, p, seed, ctx)
    print("O rel", f"{_rel(o, o_ref):.3e}")
    assert _rel(o, o_ref) <= 1e-2, _rel(o, o_ref)
    errs = {n: _rel(a, w) for n, a, w in zip(GNAMES, got, ref)}
    print("rel. Frobenius", {n: f"{e:.3e}" for n, e in errs.items()})
    for n, e in errs.items():
        assert e <= 2e-2, (n, e)


@pytest.mark.parametrize("T", [201, 77])
@pytest.mark.parametrize("size,style", WINDOWS)
def test_softmax_ctx_matches_float64(T, size, style):
    """kdfm_relpos_softmax_ctx_fwd against a float64 softmax of the same f32 scores with the banded mask: P
    within 1e-5 absolute, masked entries (outside the window, padded keys, padded query rows) exactly 0 in P
    and P_drop, P_drop either 0 or P / (1 - p) and about p of the live entries dropped."""
    from kdfm import kernels as K
    B, H, p = 3, 2, 0.1
    g = torch.Generator(device="cuda").manual_seed(T)
    ac = 3.0 * torch.randn(B, H, T, T, device="cuda", generator=g)
    bd = 3.0 * torch.randn(B, H, T, 2 * T - 1, device="cuda", generator=g)
    lens = torch.tensor(_lens(B, T), dtype=torch.int64, device="cuda")
    seed = torch.tensor([31], dtype=torch.int64, device="cuda")
    P = torch.full((B, H, T, T), float("nan"), device="cuda")
    Pd = torch.full((B, H, T, T), float("nan"), device="cuda")
    K.relpos_softmax_ctx_fwd(ac, bd, lens, P, Pd, B, H, T, 0.15, p, seed, 11, _triple(size, style))
    torch.cuda.synchronize()
    idx = (T - 1 - torch.arange(T, device="cuda")[:, None] + torch.arange(T, device="cuda")[None, :])
    s = (ac.double() + torch.gather(bd.double(), 3, idx.expand(B, H, T, T))) * 0.15
    keym = torch.arange(T, device="cuda")[None, :] < lens[:, None]
    vis = (keym[:, None, None, :] & keym[:, None, :, None] & _window(T, size, style)[None, None]).expand(B, H, T, T)
    want = torch.softmax(s.masked_fill(~vis, float("-inf")), -1)
    want = torch.where(keym[:, None, :, None], want, torch.zeros_like(want))
    assert (P.double() - want).abs().max().item() <= 1e-5
    assert (P[~vis] == 0).all() and (Pd[~vis] == 0).all()
    kept = Pd != 0
    assert (Pd[kept] - P[kept] / (1 - p)).abs().max().item() <= 1e-6
    live = vis & (P > 1e-6)
    frac = (live & ~kept).double().sum().item() / max(1.0, live.double().sum().item())
    if live.sum().item() > 2000:
        assert 0.07 < frac < 0.13, frac


@pytest.mark.parametrize("B,H,T,d", SHAPES)
@pytest.mark.parametrize("size,style", [((40, 20), "regular"), ((1, 0), "regular"), ((16, -1), "regular"),
                                        ((48, 15), "chunked_limited")])
def test_ctx_poisoned_buffers_and_determinism(B, H, T, d, size, style):
    """dS, Pd, the dPpos workspace, O, lse and every gradient output are filled with NaN before the calls: no
    output contains a NaN (no kernel reads a dS / Pd tile that no kernel wrote), and two runs are bitwise
    identical (no atomics)."""
    from kdfm import kernels as K
    seed = torch.tensor([77], dtype=torch.int64, device="cuda")
    ctx = _triple(size, style)
    one = _ctx_run(K, B, H, T, d, 0.1, seed, ctx, poison=True)
    two = _ctx_run(K, B, H, T, d, 0.1, seed, ctx, poison=True)
    for name, a, b in zip(("O", "lse") + GNAMES, one, two):
        assert not torch.isnan(a).any(), name
        assert torch.equal(a, b), name
