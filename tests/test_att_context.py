"""Limited attention context on the host side (no device): the config helper's kernel triple for both
styles, the reference's invalid combinations (conformer_encoder.py:860-880), the options the NeMo-style
ConformerEncoder refuses instead of ignoring, and the per-query interval form the kernels walk against the
dense mask the reference builds (_create_masks, :796-850), written as a predicate on index differences."""
import pytest
import torch


def test_triple_regular_and_chunked():
    from kdfm.config import FULL_CONTEXT, Ver5Config, att_context, att_context_triple
    assert att_context_triple() == FULL_CONTEXT == (-1, -1, 0)
    assert att_context(Ver5Config()) == FULL_CONTEXT
    assert att_context_triple((40, 20)) == (40, 20, 0)
    assert att_context_triple([-1, 0], "regular") == (-1, 0, 0)
    assert att_context_triple((16, -1), "regular") == (16, -1, 0)
    # chunked_limited: chunk = right + 1, left counted in chunks
    assert att_context_triple((48, 15), "chunked_limited") == (3, 15, 16)
    assert att_context_triple((128, 31), "chunked_limited") == (4, 31, 32)
    assert att_context_triple((-1, 15), "chunked_limited") == (-1, 15, 16)
    assert att_context_triple((0, 0), "chunked_limited") == (0, 0, 1)
    # chunked_limited without a right limit is the regular window
    assert att_context_triple((16, -1), "chunked_limited") == (16, -1, 0)
    assert att_context(Ver5Config(att_context_size=(48, 15), att_context_style="chunked_limited")) == (3, 15, 16)


def test_invalid_contexts_raise_value_error():
    from kdfm.config import att_context_triple
    with pytest.raises(ValueError):
        att_context_triple((40, 15), "chunked_limited")     # L % (R + 1) != 0
    with pytest.raises(ValueError):
        att_context_triple((-2, 0))
    with pytest.raises(ValueError):
        att_context_triple((4, -3), "chunked_limited")
    with pytest.raises(ValueError):
        att_context_triple((4, 4), "sliding")
    with pytest.raises(ValueError):
        att_context_triple((4,))


def _dense_mask(T, size, style):
    """The window as a dense (T, T) predicate on index differences (True = visible): regular -R <= i - j <= L;
    chunked_limited with a right limit 0 <= i // chunk - j // chunk <= L // chunk, chunk = R + 1."""
    L, R = size
    i = torch.arange(T)[:, None]
    j = torch.arange(T)[None, :]
    if style == "chunked_limited" and R >= 0:
        dc = i // (R + 1) - j // (R + 1)
        return (dc >= 0) & ((dc <= L // (R + 1)) if L >= 0 else torch.ones_like(dc, dtype=torch.bool))
    ok = torch.ones(T, T, dtype=torch.bool)
    if L >= 0:
        ok &= (i - j) <= L
    if R >= 0:
        ok &= (j - i) <= R
    return ok


@pytest.mark.parametrize("T", [1, 7, 65, 130, 201])
def test_kernel_triple_intervals_equal_reference_mask(T):
    """The (left, right, chunk) interval form the kernels walk (kernels._ctx_bounds, csrc/attn_ctx.h) equals
    the dense mask, and the visited-tile count the traces report covers exactly the tiles a visible
    pair falls in."""
    from kdfm.config import att_context_triple
    from kdfm.kernels import _ctx_bounds, ctx_tiles
    cases = [((0, 0), "regular"), ((1, 0), "regular"), ((40, 20), "regular"), ((64, 63), "regular"),
             ((-1, 0), "regular"), ((16, -1), "regular"), ((-1, -1), "regular"), ((48, 15), "chunked_limited"),
             ((128, 31), "chunked_limited"), ((-1, 7), "chunked_limited"), ((16, -1), "chunked_limited")]
    for size, style in cases:
        ctx = att_context_triple(size, style)
        got = torch.zeros(T, T, dtype=torch.bool)
        for i in range(T):
            lo, hi = _ctx_bounds(ctx, i, T)
            got[i, lo:hi + 1] = True
        want = _dense_mask(T, size, style)
        assert torch.equal(got, want), (size, style)
        nb = (T + 63) // 64
        tiles = want.new_zeros(nb, nb)
        for qb in range(nb):
            lo, _ = _ctx_bounds(ctx, qb * 64, T)
            _, hi = _ctx_bounds(ctx, min(qb * 64 + 63, T - 1), T)
            tiles[qb, lo // 64:hi // 64 + 1] = True
        hit = torch.nn.functional.max_pool2d(want[None, None].float(), 64, ceil_mode=True)[0, 0] > 0
        assert (tiles | ~hit).all(), (size, style)    # every tile with a visible pair is visited
        assert int(tiles.sum()) == ctx_tiles(T, ctx)


def test_encoder_refuses_what_it_does_not_implement():
    from kdfm import nemo
    from kdfm._lib import KdfmError
    kw = dict(n_layers=1, d_model=88, n_heads=2)
    with pytest.raises(KdfmError):
        nemo.ConformerEncoder(att_context_size=[[40, 20], [40, 0]], **kw)
    with pytest.raises(KdfmError):
        nemo.ConformerEncoder(att_context_size=[40, 20], att_context_probs=[1.0], **kw)
    with pytest.raises(KdfmError):
        nemo.ConformerEncoder(self_attention_model="rel_pos_local_attn", att_context_size=[40, 20], **kw)
    with pytest.raises(KdfmError):
        nemo.ConformerEncoder(conv_context_size=[30, 0], **kw)
    with pytest.raises(ValueError):
        nemo.ConformerEncoder(att_context_size=[40, 15], att_context_style="chunked_limited", **kw)
    with pytest.raises(ValueError):
        nemo.ConformerEncoder(att_context_size=[-2, 0], **kw)
    enc = nemo.ConformerEncoder(att_context_size=[48, 15], att_context_style="chunked_limited", **kw)
    assert enc.cfg.att_context_size == (48, 15) and enc.cfg.att_context_style == "chunked_limited"
    assert nemo.ConformerEncoder(att_context_size=[[40, 20]], **kw).cfg.att_context_size == (40, 20)
    assert nemo.ConformerEncoder(**kw).cfg.att_context_size == (-1, -1)


def test_shapes_route_only_a_binding_window():
    """EncoderShapes.ctx: None (the unchanged full-context path) for the default and for any window that covers
    the sequence; the kernel triple otherwise."""
    from kdfm.config import FULL_CONTEXT, Ver5Config
    from kdfm.conformer import EncoderShapes
    Tm = 801   # -> T = 201
    assert EncoderShapes(Ver5Config(), 2, Tm, 88, 2).ctx is None
    assert EncoderShapes(Ver5Config(att_context_size=(10 ** 6, 10 ** 6)), 2, Tm, 88, 2).ctx is None
    assert EncoderShapes(Ver5Config(att_context_size=(200, -1)), 2, Tm, 88, 2).ctx is None
    assert EncoderShapes(Ver5Config(att_context_size=(40, 20)), 2, Tm, 88, 2).ctx == (40, 20, 0)
    assert EncoderShapes(Ver5Config(att_context_size=(199, -1)), 2, Tm, 88, 2).ctx == (199, -1, 0)
    cfg = Ver5Config(att_context_size=(48, 15), att_context_style="chunked_limited")
    assert EncoderShapes(cfg, 2, Tm, 88, 2).ctx == (3, 15, 16)
    assert EncoderShapes(cfg, 2, Tm, 176, 4, ctx=FULL_CONTEXT).ctx is None    # the engine's teacher
