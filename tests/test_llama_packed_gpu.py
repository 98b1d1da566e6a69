"""Llama on a packed batch, end to end on the GPU: the fused bf16 path (document-masked flash
attention kernels + rope with positions) against the fp32 reference ops, with the bf16 reference
ops as the yardstick for what bf16 rounding alone costs; packing invariance on the fused path."""
import copy

import pytest
import torch
import torch.nn.functional as F

import distributeddataparallel_amd as xddp
from distributeddataparallel_amd.data import packed_docs_from_ids, packed_labels
from distributeddataparallel_amd.models.llama import llama_tiny

pytestmark = pytest.mark.gpu

S = 192
LAYOUTS = [[70, 122], [192]]
GRADS = ("tok_embeddings.weight", "layers.0.attention.wq.weight", "layers.0.attention.wk.weight")


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


@pytest.fixture(scope="module")
def runs():
    """(loss, logits, grads) of the three runs on the same weights and the same packed batch, and
    how many kernel forwards got a doc_start in each."""
    torch.manual_seed(0)
    # head dim 64, so the flash kernels are taken (llama_tiny's default head dim 16 falls back)
    base = llama_tiny(dim=256, n_heads=4, n_kv_heads=2, ffn_dim=512, max_seq_len=256).cuda()
    ids = torch.tensor([[i for i, n in enumerate(lens) for _ in range(n)] for lens in LAYOUTS])
    docs = packed_docs_from_ids(ids).to("cuda")
    tokens = torch.randint(0, 512, (2, S), device="cuda")
    labels = packed_labels(tokens, docs)
    C = xddp.native()
    orig = C.flash_attn_forward
    calls = {"doc": 0}

    def counted(*a, **kw):
        if len(a) > 5 and a[5] is not None or kw.get("doc_start") is not None:
            calls["doc"] += 1
        return orig(*a, **kw)

    mp = pytest.MonkeyPatch()
    mp.setattr(C, "flash_attn_forward", counted)
    out = {}
    try:
        for name, dtype, fused in (("fp32_ref", torch.float32, "0"), ("bf16_ref", torch.bfloat16, "0"),
                                   ("bf16_fused", torch.bfloat16, "1")):
            mp.setenv("XDDP_FUSED_TRANSFORMER", fused)
            m = copy.deepcopy(base).to(dtype)
            calls["doc"] = 0
            logits = m(tokens, docs)
            loss = F.cross_entropy(logits.float().flatten(0, 1), labels.flatten(), ignore_index=-100)
            loss.backward()
            grads = {n: p.grad.detach().float() for n, p in m.named_parameters() if n in GRADS}
            out[name] = (loss.item(), logits.detach().float(), grads, calls["doc"])
            if name == "bf16_fused":  # document 1 of row 0 alone, on the same path
                a = LAYOUTS[0][0]
                with torch.no_grad():
                    out["alone"] = (m(tokens[:1, a:]).float(), a)
    finally:
        mp.undo()
    return out


def test_packed_fused_within_bf16_rounding_of_fp32_reference(runs):
    """Error of the fused bf16 run against the fp32 reference <= 2x the bf16 reference ops' error
    against it (+ 1e-6): both are bf16 pipelines that differ in rounding order only, and the factor
    2 is the allowance for that. Measured on MI355X (bf16 reference | fused): loss error 3.1e-5 |
    2.7e-5; relative gradient error tok_embeddings 9.5e-3 | 8.9e-3, wq 1.11e-2 | 1.06e-2,
    wk 1.14e-2 | 1.07e-2."""
    l1, _, g1, _ = runs["fp32_ref"]
    l2, _, g2, _ = runs["bf16_ref"]
    l3, _, g3, _ = runs["bf16_fused"]
    e2, e3 = abs(l2 - l1), abs(l3 - l1)
    print(f"loss fp32 {l1:.6f} | bf16 ref err {e2:.3e} | bf16 fused err {e3:.3e}")
    fails = [] if e3 <= 2 * e2 + 1e-6 else [("loss", e3, e2)]
    for n in GRADS:
        e2, e3 = _rel(g2[n], g1[n]), _rel(g3[n], g1[n])
        print(f"grad {n}: bf16 ref rel err {e2:.3e} | bf16 fused rel err {e3:.3e}")
        if not e3 <= 2 * e2 + 1e-6:
            fails.append((n, e3, e2))
    assert not fails, fails


def test_packed_fused_packing_invariance(runs):
    """Document 1 of row 0 alone gives the logits of its rows in the packed run, to within the
    margin measured above for those rows: 2x the bf16 reference ops' error against fp32 (+ 1e-6).
    Alone and packed are the same bf16 math in another tile order. Measured on MI355X: 3.2e-3
    against a bf16-reference error of 7.1e-3 on those rows."""
    alone, a = runs["alone"]
    packed = runs["bf16_fused"][1][:1, a:]
    margin = _rel(runs["bf16_ref"][1][:1, a:], runs["fp32_ref"][1][:1, a:])
    err = _rel(alone, packed)
    print(f"alone vs packed rel err {err:.3e} | bf16 ref vs fp32 on the same rows {margin:.3e}")
    assert err <= 2 * margin + 1e-6, (err, margin)


def test_packed_fused_run_called_the_doc_kernels(runs):
    n_layers = 2
    assert runs["bf16_fused"][3] == n_layers, runs["bf16_fused"][3]
    assert runs["fp32_ref"][3] == 0 and runs["bf16_ref"][3] == 0
