"""Limited attention context (att_context_size / att_context_style) through the public interfaces on the GPU:
the NeMo-style kdfm.nemo.ConformerEncoder and the fused Ver5Engine (student encoder; the teacher stays
full-context) against a float64 composition of the oracle's subsampling / conformer_layer with the banded
attention mask -- the per-query interval form
  regular (L, R):          query i sees keys [i - L, i + R] (-1: unlimited),
  chunked_limited (L, R):  chunk = R + 1, c = i // chunk, keys [(c - L // chunk) chunk, (c + 1) chunk - 1],
AND-ed with the padding square, then inverted (True = masked), as the reference's _create_masks builds it.

Tolerances: f32 math as tests/test_nemo_api_gpu.py::test_module_training_step_matches_oracle (outputs 2e-4
relative + 1e-4; a gradient passes at 2e-3 of its max or within 4x the float32 oracle's own distance to
float64); bf16 math as tests/test_step_parity_gpu.py (layer outputs rel. Frobenius 1.5e-2, gradients rel.
Frobenius max(5e-2, 2.5 x the oracle's own sensitivity to bf16-rounded weights)); engine inference log-probs at
the smoke tolerance (rtol 2e-4, atol 2e-4)."""
import math
from dataclasses import replace

import pytest
import torch

from oracle import ver5 as O

pytestmark = pytest.mark.gpu


def _banded_att_mask(T, lengths, size, style):
    """(B, T, T) bool, True = masked."""
    L, R = size
    i = torch.arange(T)
    if style == "chunked_limited" and R >= 0:
        chunk = R + 1
        c = i // chunk
        lo = torch.zeros_like(i) if L < 0 else (c - L // chunk) * chunk
        hi = (c + 1) * chunk - 1
    else:
        lo = torch.zeros_like(i) if L < 0 else i - L
        hi = torch.full_like(i, T - 1) if R < 0 else i + R
    j = i[None, :]
    window = (j >= lo[:, None]) & (j <= hi[:, None])
    valid = torch.arange(T).expand(len(lengths), T) < lengths.unsqueeze(1)
    square = valid.unsqueeze(1) & valid.unsqueeze(2)
    return ~(square & window.unsqueeze(0))


def _oracle_encoder(mel_bft, lengths, p, prefix, d, h, ocfg, training, bn_state, size, style):
    """oracle.ver5.encoder with the banded att_mask: -> (last layer (B, T, d), lengths, per-layer outputs)."""
    x, length = O.subsampling(mel_bft.transpose(1, 2), lengths, p, prefix + "pre_encode.", ocfg)
    B, T, _ = x.shape
    x = x * math.sqrt(d)
    pos_emb = O.rel_pos_emb(T, d, x.dtype)
    att_mask = _banded_att_mask(T, length, size, style)
    pad_mask = ~(torch.arange(T).expand(B, T) < length.unsqueeze(1))
    feats = []
    for i in range(ocfg.n_layers):
        x = O.conformer_layer(x, pos_emb, att_mask, pad_mask, p, prefix + f"layers.{i}.", h, training, bn_state, ocfg)
        feats.append(x)
    return x, length, feats


def _module_case(size, style, mode):
    from kdfm import kernels as K
    from kdfm import nemo
    K.set_math(mode)
    K.set_deterministic(True)   # ordered reductions (restored by the conftest fixture)
    n_layers, d, h, B, Tm = 2, 88, 2, 3, 201   # about 2 s of features -> T = 51 frames
    enc = nemo.ConformerEncoder(n_layers=n_layers, d_model=d, n_heads=h, att_context_size=list(size),
                                att_context_style=style, dropout=0.0, dropout_pre_encoder=0.0, dropout_att=0.0,
                                device="cuda", init_seed=3)
    enc.train()
    g = torch.Generator().manual_seed(17)
    mel = torch.randn(B, 80, Tm, generator=g)
    lens = torch.tensor([Tm, 163, 58], dtype=torch.int64)
    for bi in range(B):
        mel[bi, :, int(lens[bi]):] = 0.0
    sd = {k: v.detach().cpu().clone() for k, v in enc.state_dict().items()}
    out, olen = enc(audio_signal=mel.cuda(), length=lens.cuda())
    T = out.shape[2]
    w = torch.randn(B, d, T, generator=g)
    valid = (torch.arange(T).expand(B, T) < olen.cpu().unsqueeze(1))
    w = w * valid.unsqueeze(1)
    (out * w.cuda()).sum().backward()
    torch.cuda.synchronize()

    ocfg = O.StepConfig(n_layers=n_layers)
    names = [k for k in sd if "running_" not in k and "num_batches" not in k]

    def run(dtype, rounded=False):
        p = {}
        for k, v in sd.items():
            v = v.to(dtype) if v.is_floating_point() else v
            if rounded and k in names and v.dim() >= 2:
                v = v.bfloat16().to(dtype)
            p[k] = v.clone().requires_grad_(True) if k in names else v.clone()
        bn = {k: v.clone() for k, v in p.items() if "running_" in k}
        x, length, _ = _oracle_encoder(mel.to(dtype), lens, p, "", d, h, ocfg, True, bn, size, style)
        loss = (x.transpose(1, 2) * w.to(dtype)).sum()
        grads = torch.autograd.grad(loss, [p[k] for k in names], allow_unused=True)
        return x.detach().transpose(1, 2), length, grads

    ref, rlen, og = run(torch.float64)
    assert torch.equal(olen.cpu(), rlen)
    params = dict(enc.named_parameters())
    got_o = (out.detach().cpu().double() * valid.unsqueeze(1))
    ref_o = ref * valid.unsqueeze(1)
    checked = 0
    if mode == "f32":
        _, _, og32 = run(torch.float32)
        err = (got_o - ref_o).abs().max().item()
        print(f"output max err {err:.3e} (max |ref| {ref_o.abs().max().item():.3e})")
        assert err <= 2e-4 * ref_o.abs().max().item() + 1e-4, err
        for k, gr, g32 in zip(names, og, og32):
            if gr is None or k.endswith(("self_attn.linear_k.bias", "conv.depthwise_conv.bias")):
                continue
            mine = params[k].grad
            assert mine is not None, k
            e = (mine.detach().cpu().double() - gr).abs().max().item()
            noise = (g32.double() - gr).abs().max().item() if g32 is not None else 0.0
            assert e <= 2e-3 * gr.abs().max().item() + 1e-6 or e <= 4.0 * noise, (k, e, noise)
            checked += 1
    else:
        def frob(a, b):
            return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()
        ref_b, _, ogb = run(torch.float64, rounded=True)
        sens_o = frob(ref_b * valid.unsqueeze(1), ref_o)
        e = frob(got_o, ref_o)
        print(f"output rel. Frobenius {e:.3e}, sensitivity {sens_o:.3e}")
        assert e <= max(1.5e-2, 2.5 * sens_o), (e, sens_o)
        for k, gr, gb in zip(names, og, ogb):
            if gr is None or k.endswith(("self_attn.linear_k.bias", "conv.depthwise_conv.bias")):
                continue
            mine = params[k].grad
            assert mine is not None, k
            e = frob(mine.detach().cpu().double(), gr)
            sens = frob(gb, gr)
            assert e <= max(5e-2, 2.5 * sens), (k, e, sens)
            checked += 1
    assert checked > 60


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("size,style", [((40, 20), "regular"), ((48, 15), "chunked_limited")])
def test_module_limited_context_matches_oracle(size, style, mode):
    """ConformerEncoder(att_context_size=..., att_context_style=...) in training mode (batch-statistics
    BatchNorm, no dropout), B = 3 ragged utterances of about 2 s: output on the valid frames and every parameter
    gradient against the float64 oracle loop with the banded mask (tolerances: module docstring)."""
    _module_case(size, style, mode)


def _oracle_infer(eng, wav, wl, size, style, dtype=torch.float64):
    cfg = eng.cfg
    ocfg = O.StepConfig(n_layers=cfg.n_layers)
    p = {}
    p.update(O.frontend_buffers(ocfg))
    p.update(eng.student.state_dict())
    bn = {name: eng.bn.P[name].detach().cpu().clone() for name, _ in eng.bn.specs}
    p.update(bn)
    p = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in p.items()}
    mel, mel_len = O.preprocess(wav.to(dtype), wl, p["preprocessor.featurizer.window"],
                                p["preprocessor.featurizer.fb"][0], ocfg)
    x, olen, _ = _oracle_encoder(mel, mel_len, p, "encoder.", ocfg.d_student, ocfg.heads_student, ocfg, False,
                                 {k: v.to(dtype) for k, v in bn.items()}, size, style)
    return O.decoder(x.transpose(1, 2), p, "decoder."), olen


def _batch(cfg, B=3, N=32000, U=8):
    g = torch.Generator().manual_seed(5)
    wav = 0.1 * torch.randn(B, N, generator=g)
    wl = torch.tensor([N, N - 2400, 20000][:B], dtype=torch.int64)
    tg = torch.randint(0, cfg.vocab, (B, U), generator=g)
    tl = torch.tensor([U, U - 3, 4][:B], dtype=torch.int64)
    return wav, wl, tg, tl


def test_engine_infer_matches_oracle_with_limited_context():
    """Ver5Config(att_context_size=(40, 20)).parity(): the student's inference log-probs on the valid frames
    against the float64 composition (frontend, banded-mask encoder loop, decoder), rtol / atol 2e-4."""
    from kdfm.config import Ver5Config
    from kdfm.engine import Ver5Engine
    size = (40, 20)
    cfg = Ver5Config(n_layers=2, att_context_size=size).parity()
    eng = Ver5Engine(cfg, "cuda:0")
    wav, wl, _, _ = _batch(cfg)
    lp, enc_len = eng.infer(wav.cuda(), wl.cuda())
    ref, olen = _oracle_infer(eng, wav, wl, size, "regular")
    assert torch.equal(enc_len.cpu(), olen)
    assert lp.shape[1] == 51   # the window binds: 51 frames > 40 + 1
    for bi in range(wav.shape[0]):
        L = int(olen[bi])
        torch.testing.assert_close(lp[bi, :L].cpu().double(), ref[bi, :L], rtol=2e-4, atol=2e-4)
    # the window matters: the full-context engine with the same weights computes something else
    full = Ver5Engine(replace(cfg, att_context_size=(-1, -1)), "cuda:0")
    lp_full, _ = full.infer(wav.cuda(), wl.cuda())
    assert (lp_full - lp).abs().max().item() > 1e-3


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_engine_training_step_and_plan_with_limited_context(mode):
    """One training step with att_context_size=(40, 20) runs with finite losses and gradients, and a recorded
    step plan replays bitwise equal to the eager steps (parameters, AdamW moments, BatchNorm statistics), in
    the f32 parity route (relpos_softmax_ctx_fwd) and the bf16 route (the windowed fused kernels)."""
    from kdfm.config import Ver5Config
    from kdfm.engine import Ver5Engine
    cfg = replace(Ver5Config(n_layers=2, att_context_size=(40, 20)).parity(), math=mode)
    wav, wl, tg, tl = (t.cuda() for t in _batch(cfg))

    def engine():
        eng = Ver5Engine(cfg, "cuda", teacher_seed=0, student_seed=1, heads_seed=2)
        eng.set_seed(91)
        return eng
    a, b = engine(), engine()
    ctx = a.forward(wav, wl, tg, tl, train=True)
    a.backward(ctx)
    torch.cuda.synchronize()
    assert torch.isfinite(a.losses).all() and torch.isfinite(a.student.grad).all()
    assert a.student.grad.abs().max().item() > 0
    a, b = engine(), engine()
    a.train_step(wav, wl, tg, tl)       # warm-up step on both: lazily created workspaces
    b.train_step(wav, wl, tg, tl)
    plan = b.make_plan(wav, wl, tg, tl)   # the recording is step 2 of b
    a.train_step(wav, wl, tg, tl)
    for _ in range(2):
        a.train_step(wav, wl, tg, tl)
        plan.replay()
    torch.cuda.synchronize()
    torch.testing.assert_close(a.losses, b.losses, rtol=1e-5, atol=0.0)
    for name in ("data", "exp_avg", "exp_avg_sq"):
        x, y = getattr(a.student, name), getattr(b.student, name)
        assert torch.equal(x, y), f"student.{name} differs: {(x - y).abs().max().item():.3e}"
    assert torch.equal(a.bn.data, b.bn.data)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_engine_covering_window_is_bitwise_default(mode):
    """att_context_size=(10**6, 10**6) covers every sequence: the hooked layer outputs and every gradient are
    bitwise the default config's in deterministic mode (the same code path and kernels).  The five scalar
    losses keep float-atomic accumulators even in deterministic mode (tests/test_determinism_gpu.py: two runs of
    ONE config agree to 1e-5 relative, not bitwise), so they are compared at that project bound."""
    from kdfm.config import Ver5Config
    from kdfm.engine import Ver5Engine
    base = replace(Ver5Config(n_layers=2).parity(), math=mode)
    wav, wl, tg, tl = (t.cuda() for t in _batch(base))
    res = []
    for cfg in (base, replace(base, att_context_size=(10 ** 6, 10 ** 6))):
        eng = Ver5Engine(cfg, "cuda", teacher_seed=0, student_seed=1, heads_seed=2)
        eng.set_seed(91)
        ctx = eng.forward(wav, wl, tg, tl, train=True)
        feats = ctx["sfeats"].clone()
        eng.backward(ctx)
        torch.cuda.synchronize()
        res.append((eng.losses.clone(), eng.student.grad.clone(), feats))
    print("losses bitwise equal:", torch.equal(res[0][0], res[1][0]))
    torch.testing.assert_close(res[0][0], res[1][0], rtol=1e-5, atol=0.0)
    assert torch.equal(res[0][2], res[1][2])
    assert torch.equal(res[0][1], res[1][1])
