"""Packed sequences on the CPU: the per-token document bounds (data/packing.py), the labels, the
document-masked attention fallback and the Llama model's packing invariance — a document inside a
packed row must give the logits it gives alone (positions restart, attention stops at its edges)."""
import math

import pytest
import torch
import torch.nn.functional as F

from distributeddataparallel_amd.data import PackedDocs, packed_docs, packed_docs_from_ids, packed_labels
from distributeddataparallel_amd.models.llama import llama_tiny
from distributeddataparallel_amd.ops.attention import flash_attention
from distributeddataparallel_amd.ops.transformer import rope, rope_reference

EOS = 9
IGN = -100

# (tokens, doc_start, doc_end, positions, doc ids, labels)
ROWS = {
    "eos_middle": ([1, 2, EOS, 3, 4, 5], [0, 0, 0, 3, 3, 3], [3, 3, 3, 6, 6, 6], [0, 1, 2, 0, 1, 2],
                   [0, 0, 0, 1, 1, 1], [2, EOS, IGN, 4, 5, IGN]),
    "two_eos": ([1, EOS, EOS, 2, 3, 4], [0, 0, 2, 3, 3, 3], [2, 2, 3, 6, 6, 6], [0, 1, 0, 0, 1, 2],
                [0, 0, 1, 2, 2, 2], [EOS, IGN, IGN, 3, 4, IGN]),
    "eos_last": ([1, 2, 3, 4, 5, EOS], [0] * 6, [6] * 6, [0, 1, 2, 3, 4, 5], [4] * 6, [2, 3, 4, 5, EOS, IGN]),
    "no_eos": ([1, 2, 3, 4, 5, 6], [0] * 6, [6] * 6, [0, 1, 2, 3, 4, 5], [0] * 6, [2, 3, 4, 5, 6, IGN]),
    "eos_first": ([EOS, 1, 2, EOS, 3, 4], [0, 1, 1, 1, 4, 4], [1, 4, 4, 4, 6, 6], [0, 0, 1, 2, 0, 1],
                  [7, 3, 3, 3, 5, 5], [IGN, 2, EOS, IGN, 4, IGN]),
}
BATCHES = [[n] for n in ROWS] + [["eos_middle", "two_eos"], ["no_eos", "eos_first"]]


def _batch(names, col):
    return torch.tensor([ROWS[n][col] for n in names])


@pytest.mark.parametrize("names", BATCHES, ids=["+".join(b) for b in BATCHES])
def test_packed_docs_bounds(names):
    tokens = _batch(names, 0)
    d = packed_docs(tokens, EOS)
    assert isinstance(d, PackedDocs)
    for got, col in ((d.doc_start, 1), (d.doc_end, 2), (d.positions, 3)):
        assert got.dtype == torch.int32 and got.shape == tokens.shape and got.is_contiguous()
        assert torch.equal(got, _batch(names, col).to(torch.int32))
    e = packed_docs_from_ids(_batch(names, 4))
    for a, b in zip(d, e):
        assert a.dtype == b.dtype and torch.equal(a, b)
    moved = d.to("cpu")
    assert isinstance(moved, PackedDocs) and all(torch.equal(a, b) for a, b in zip(d, moved))


@pytest.mark.parametrize("names", BATCHES, ids=["+".join(b) for b in BATCHES])
def test_packed_labels(names):
    tokens = _batch(names, 0)
    labels = packed_labels(tokens, packed_docs(tokens, EOS))
    assert labels.dtype == tokens.dtype
    assert torch.equal(labels, _batch(names, 5))
    assert torch.equal(packed_labels(tokens, packed_docs(tokens, EOS), ignore_index=-1),
                       _batch(names, 5).masked_fill(_batch(names, 5) == IGN, -1))


def _docs_of(lengths_per_row, S):
    ids = torch.tensor([[i for i, n in enumerate(lens) for _ in range(n)] for lens in lengths_per_row])
    assert ids.shape[1] == S
    return packed_docs_from_ids(ids)


def test_flash_attention_docs_cpu_matches_per_document():
    torch.manual_seed(0)
    B, S, H, Hkv, D = 2, 24, 4, 2, 16
    layouts = [[5, 1, 18], [24]]
    docs = _docs_of(layouts, S)
    q = torch.randn(B, S, H, D)
    k = torch.randn(B, S, Hkv, D)
    v = torch.randn(B, S, Hkv, D)
    o = flash_attention(q, k, v, causal=True, docs=docs)
    assert o.shape == (B, S, H, D)
    for b, lens in enumerate(layouts):
        a = 0
        for n in lens:
            ref = flash_attention(q[b:b + 1, a:a + n], k[b:b + 1, a:a + n], v[b:b + 1, a:a + n], causal=True)
            torch.testing.assert_close(o[b:b + 1, a:a + n], ref, rtol=1e-4, atol=1e-5)
            a += n
    # non-causal: same-document membership
    o2 = flash_attention(q, k, v, causal=False, docs=docs)
    ref = flash_attention(q[:1, 6:24], k[:1, 6:24], v[:1, 6:24], causal=False)
    torch.testing.assert_close(o2[:1, 6:24], ref, rtol=1e-4, atol=1e-5)
    # the dense form of the same mask, written out independently
    scale = 1.0 / math.sqrt(D)
    kk = k.repeat_interleave(H // Hkv, dim=2)
    vv = v.repeat_interleave(H // Hkv, dim=2)
    s = torch.einsum("bqhd,bkhd->bhqk", q, kk) * scale
    idx = torch.arange(S)
    vis = (idx[None, None, :] >= docs.doc_start[:, :, None]) & (idx[None, None, :] <= idx[None, :, None])
    p = s.masked_fill(~vis[:, None], float("-inf")).softmax(-1)
    torch.testing.assert_close(o, torch.einsum("bhqk,bkhd->bqhd", p, vv), rtol=1e-4, atol=1e-5)


def test_llama_packing_invariance_cpu():
    torch.manual_seed(0)
    model = llama_tiny().eval()
    S = 40
    layouts = [[7, 1, 32], [40]]
    tokens = torch.randint(0, 512, (2, S))
    docs = _docs_of(layouts, S)
    with torch.no_grad():
        packed = model(tokens, docs)
        for b, lens in enumerate(layouts):
            a = 0
            for n in lens:
                alone = model(tokens[b:b + 1, a:a + n])
                torch.testing.assert_close(packed[b:b + 1, a:a + n], alone, rtol=1e-4, atol=1e-5)
                a += n
        # and the mask matters: without docs the second document of row 0 sees the first
        assert not torch.allclose(model(tokens)[0, 8:], packed[0, 8:], rtol=1e-4, atol=1e-5)


def test_llama_packed_backward_cpu():
    """The packed loss (packed_labels' ignore_index) equals the per-document losses' token-weighted
    mean, and its gradients match."""
    torch.manual_seed(1)
    model = llama_tiny()
    S = 24
    lens = [9, 15]
    tokens = torch.randint(0, 512, (1, S))
    docs = _docs_of([lens], S)
    labels = packed_labels(tokens, docs)
    loss = F.cross_entropy(model(tokens, docs).flatten(0, 1), labels.flatten(), ignore_index=IGN)
    loss.backward()
    g_packed = model.layers[0].attention.wq.weight.grad.clone()
    model.zero_grad()
    total, a = 0.0, 0
    for n in lens:
        t = tokens[:, a:a + n]
        total = total + F.cross_entropy(model(t)[:, :-1].flatten(0, 1), t[:, 1:].flatten(), reduction="sum")
        a += n
    ref = total / (S - len(lens))
    ref.backward()
    torch.testing.assert_close(loss, ref, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(g_packed, model.layers[0].attention.wq.weight.grad, rtol=1e-4, atol=1e-5)


def test_plain_path_unchanged():
    torch.manual_seed(0)
    model = llama_tiny().eval()
    tokens = torch.randint(0, 512, (2, 16))
    with torch.no_grad():
        assert torch.equal(model(tokens), model(tokens, docs=None))
    x = torch.randn(2, 16, 4, 16)
    cos, sin = model._tables(x.device)
    assert torch.equal(rope(x, cos, sin), rope(x, cos, sin, positions=None))
    assert torch.equal(rope_reference(x, cos, sin), rope_reference(x, cos, sin, None))
    pos = torch.arange(16, dtype=torch.int32).expand(2, 16).contiguous()
    assert torch.equal(rope(x, cos, sin), rope(x, cos, sin, pos))
    q = torch.randn(2, 16, 4, 16)
    assert torch.equal(flash_attention(q, q, q, causal=True), flash_attention(q, q, q, causal=True, docs=None))
