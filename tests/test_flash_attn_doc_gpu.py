"""Document-masked causal flash attention (the DOC variants of csrc/kernels/flash_attn.hip) vs an
fp32 PyTorch reference of the same math with the document mask, on layouts that reach every
variant and every skipping rule; bitwise guards (one document = plain causal, isolation between
documents, repeatability); rope with per-token positions; the SDPA fallback."""
import math

import pytest
import torch

import distributeddataparallel_amd as xddp
from distributeddataparallel_amd.data import packed_docs_from_ids
from distributeddataparallel_amd.ops.attention import flash_attention
from distributeddataparallel_amd.ops.transformer import rope, rope_reference

pytestmark = pytest.mark.gpu


def _docs(layouts, S, device="cuda"):
    """layouts: document lengths per batch row."""
    ids = torch.tensor([[i for i, n in enumerate(lens) for _ in range(n)] for lens in layouts])
    assert ids.shape[1] == S
    return packed_docs_from_ids(ids).to(device)


def _ref(q, k, v, scale, doc_start):
    B, S, H, D = q.shape
    Hkv = k.shape[2]
    qf, kf, vf = (t.float().transpose(1, 2) for t in (q, k, v))
    if Hkv != H:
        kf = kf.repeat_interleave(H // Hkv, dim=1)
        vf = vf.repeat_interleave(H // Hkv, dim=1)
    s = qf @ kf.transpose(-1, -2) * scale
    idx = torch.arange(S, device=q.device)
    m = (idx[None, None, :] <= idx[None, :, None]) & (idx[None, None, :] >= doc_start[:, :, None])  # [B, Sq, Sk]
    s = s.masked_fill(~m[:, None], float("-inf"))
    p = s.softmax(-1)
    return (p @ vf).transpose(1, 2)


def _inputs(B, S, H, Hkv, D, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    mk = lambda h: torch.randn(B, S, h, D, device="cuda", dtype=torch.bfloat16, generator=g)  # noqa: E731
    return mk(H), mk(Hkv), mk(Hkv), mk(H)


def _run(q, k, v, do, docs):
    q, k, v = (t.detach().clone().requires_grad_() for t in (q, k, v))
    o = flash_attention(q, k, v, causal=True, docs=docs)
    o.backward(do)
    return o.detach(), q.grad, k.grad, v.grad


LAYOUT3 = (1, 512, 8, 2, 128, [[100, 156, 1, 255]])


@pytest.mark.parametrize("B,S,H,Hkv,D,layouts", [
    (1, 64, 2, 1, 64, [[1, 31, 32]]),             # one tile, a 1-token document, a boundary inside a wave
    (2, 130, 4, 4, 128, [[130], [63, 2, 65]]),    # ragged S, per-row layouts, grp = 1 so nsplit = 1
    LAYOUT3,                                      # off-tile, on a 256 edge, one past it; GQA nsplit = 4; NW = 4 pairs
    (4, 512, 32, 8, 128, [[300, 212]] * 4),       # wg8 = 256: the NW = 8 forward and dQ
    (1, 384, 4, 4, 64, [[129, 255]]),             # D64 causal dK/dV with two groups
    (1, 256, 4, 2, 64, [[64, 64, 128]]),          # tile-aligned boundaries: whole-tile skips, no lower mask
])
def test_doc_attention_matches_reference(B, S, H, Hkv, D, layouts):
    docs = _docs(layouts, S)
    q, k, v, do = _inputs(B, S, H, Hkv, D)
    o, dq, dk, dv = _run(q, k, v, do, docs)
    qr, kr, vr = (t.float().requires_grad_() for t in (q, k, v))
    ref = _ref(qr, kr, vr, 1.0 / math.sqrt(D), docs.doc_start)
    assert o.shape == (B, S, H, D) and o.dtype == torch.bfloat16
    torch.testing.assert_close(o.float(), ref, rtol=2e-2, atol=2e-2)
    ref.backward(do.float())
    for name, a, b in (("dq", dq, qr.grad), ("dk", dk, kr.grad), ("dv", dv, vr.grad)):
        rel = ((a.float() - b).norm() / b.norm()).item()
        print(f"{name} rel {rel:.3e}")
        assert rel < 2e-2, (name, rel)


@pytest.mark.parametrize("B,S,H,Hkv,D", [(1, 512, 8, 2, 128), (2, 130, 4, 4, 64)])
def test_one_document_is_plain_causal_bitwise(B, S, H, Hkv, D):
    C = xddp.native()
    docs = _docs([[S]] * B, S)
    assert int(docs.doc_start.max()) == 0 and int(docs.doc_end.min()) == S
    q, k, v, do = _inputs(B, S, H, Hkv, D, seed=3)
    scale = 1.0 / math.sqrt(D)
    o0, lse0 = C.flash_attn_forward(q, k, v, True, scale)
    o1, lse1 = C.flash_attn_forward(q, k, v, True, scale, docs.doc_start)
    torch.testing.assert_close(o1, o0, rtol=0, atol=0)
    torch.testing.assert_close(lse1, lse0, rtol=0, atol=0)
    g0 = C.flash_attn_backward(do, q, k, v, o0, lse0, True, scale)
    g1 = C.flash_attn_backward(do, q, k, v, o1, lse1, True, scale, doc_start=docs.doc_start, doc_end=docs.doc_end)
    for a, b in zip(g1, g0):
        torch.testing.assert_close(a, b, rtol=0, atol=0)
    # and through the public op
    plain = _run(q, k, v, do, None)
    packed = _run(q, k, v, do, docs)
    for a, b in zip(packed, plain):
        torch.testing.assert_close(a, b, rtol=0, atol=0)


def test_documents_are_isolated_bitwise():
    B, S, H, Hkv, D, layouts = LAYOUT3
    docs = _docs(layouts, S)
    q, k, v, do = _inputs(B, S, H, Hkv, D, seed=5)
    base = _run(q, k, v, do, docs)
    n0 = layouts[0][0]
    q2, k2, v2, do2 = (t.clone() for t in (q, k, v, do))
    for t, r in zip((q2, k2, v2, do2), _inputs(B, S, H, Hkv, D, seed=6)):
        t[:, :n0] = r[:, :n0]
        assert torch.isfinite(t).all()
    assert not torch.equal(q2[:, :n0], q[:, :n0])
    other = _run(q2, k2, v2, do2, docs)
    for name, a, b in zip(("o", "dq", "dk", "dv"), other, base):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a[:, n0:], b[:, n0:]), name
        assert not torch.equal(a[:, :n0], b[:, :n0]), name


def test_doc_gradients_repeatable():
    B, S, H, Hkv, D, layouts = LAYOUT3
    docs = _docs(layouts, S)
    q, k, v, do = _inputs(B, S, H, Hkv, D, seed=7)
    for a, b in zip(_run(q, k, v, do, docs), _run(q, k, v, do, docs)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5), (torch.bfloat16, 1e-2)])
def test_rope_positions(dtype, tol):
    B, S, H, Dh = 2, 96, 4, 64
    docs = _docs([[63, 2, 31], [96]], S)
    g = torch.Generator(device="cuda").manual_seed(0)
    inv = 1.0 / (10000.0 ** (torch.arange(0, Dh, 2, dtype=torch.float32, device="cuda") / Dh))
    f = torch.outer(torch.arange(128, dtype=torch.float32, device="cuda"), inv)
    cos, sin = torch.cos(f).contiguous(), torch.sin(f).contiguous()
    x = torch.randn(B, S, H, Dh, device="cuda", dtype=dtype, generator=g)
    dy = torch.randn(B, S, H, Dh, device="cuda", dtype=dtype, generator=g)
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    y = rope(xa, cos, sin, docs.positions)
    ref = rope_reference(xb, cos, sin, docs.positions)
    assert y.dtype == dtype
    torch.testing.assert_close(y, ref, rtol=tol, atol=tol)
    # the positions are really used: a restarted row differs from the plain call, an unbroken one does not
    plain = rope(x, cos, sin)
    assert not torch.equal(y[0, 63:], plain[0, 63:])
    assert torch.equal(y[1], plain[1]) and torch.equal(y[0, :63], plain[0, :63])
    y.backward(dy)
    ref.backward(dy)
    torch.testing.assert_close(xa.grad, xb.grad, rtol=tol, atol=tol)


def test_doc_fallback_parity(monkeypatch):
    B, S, H, Hkv, D, layouts = LAYOUT3
    docs = _docs(layouts, S)
    q, k, v, _ = _inputs(B, S, H, Hkv, D, seed=9)
    o = flash_attention(q, k, v, causal=True, docs=docs)
    monkeypatch.setenv("XDDP_FLASH_ATTN", "0")
    fb = flash_attention(q, k, v, causal=True, docs=docs)
    assert fb.shape == o.shape and fb.dtype == o.dtype
    torch.testing.assert_close(o.float(), fb.float(), rtol=2e-2, atol=2e-2)
