"""The FP8 linear ops (ops/fp8.py behind ``XDDP_FP8``) on the GPU: kernels against the torch
emulation on identical inputs, the DDP gradient-target write, and a tiny Llama end to end."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _randn(*shape, std=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (std * torch.randn(*shape, generator=g)).to(torch.bfloat16).cuda()


@pytest.fixture(scope="module")
def ops_data():
    """x [2, 128, 256] (256 tokens, K = 256), weights with N = 128 / 384 / 128, a residual and the
    output gradients; shared by the tests below and never modified."""
    K = 256
    return dict(x=_randn(2, 128, K, seed=1), ws=[_randn(n, K, std=K ** -0.5, seed=10 + i) for i, n in enumerate((128, 384, 128))],
                res=_randn(2, 128, 384, seed=2), dys=[_randn(2, 128, n, seed=20 + i) for i, n in enumerate((128, 384, 128))])


def _run_ops(monkeypatch, mode, d):
    from distributeddataparallel_amd.ops.linear import linear, multi_linear

    monkeypatch.setenv("XDDP_FP8", mode)
    out = {}
    # linear with a residual (N = 384) and without (N = 128)
    for name, w, res, dy in (("lin_res", d["ws"][1], d["res"], d["dys"][1]), ("lin", d["ws"][0], None, d["dys"][0])):
        x, w = d["x"].clone().requires_grad_(True), w.clone().requires_grad_(True)
        r = None if res is None else res.clone().requires_grad_(True)
        y = linear(x, w, r)
        y.backward(dy)
        out[name] = [y.detach(), x.grad, w.grad] + ([] if r is None else [r.grad])
    # multi_linear over three weights: x quantized once, dX accumulated in the GEMM epilogue
    x = d["x"].clone().requires_grad_(True)
    ws = [w.clone().requires_grad_(True) for w in d["ws"]]
    ys = multi_linear(x, *ws)
    torch.autograd.backward(list(ys), d["dys"])
    out["multi"] = [y.detach() for y in ys] + [x.grad] + [w.grad for w in ws]
    return out


def test_ops_match_emulation(monkeypatch, ops_data):
    """Kernels vs emulation on the same GPU inputs: the quantized operands are identical, only the
    accumulation order and one bf16 rounding differ — the project's bf16 GEMM bound, 5e-3."""
    got = _run_ops(monkeypatch, "1", ops_data)
    ref = _run_ops(monkeypatch, "emulate", ops_data)
    plain = _run_ops(monkeypatch, "0", ops_data)
    for name in ref:
        for i, (a, b) in enumerate(zip(got[name], ref[name])):
            r = _rel(a, b)
            print(f"{name}[{i}]: kernel vs emulate rel {r:.2e}")
            assert a.dtype == torch.bfloat16 and a.shape == b.shape
            assert r < 5e-3, (name, i, r)
    # the FP8 path really ran: its Y differs from the bf16 path's by FP8 quantization error
    assert 0.01 < _rel(got["lin"][0], plain["lin"][0]) < 0.06
    assert torch.equal(got["lin_res"][3], ops_data["dys"][1])


def test_dw_lands_in_grad_target(monkeypatch, ops_data):
    from distributeddataparallel_amd.ops.linear import clear_grad_targets, linear, set_grad_targets

    monkeypatch.setenv("XDDP_FP8", "1")
    x = ops_data["x"].clone().requires_grad_(True)
    w = ops_data["ws"][1].clone().requires_grad_(True)
    bucket = torch.full((w.numel() + 64,), 3.0, dtype=torch.bfloat16, device="cuda")
    target = bucket[32:32 + w.numel()].view_as(w)
    set_grad_targets([w], [target])
    try:
        linear(x, w).backward(ops_data["dys"][1])
    finally:
        clear_grad_targets([w])
    assert w.grad.data_ptr() == target.data_ptr()
    assert (bucket[:32] == 3).all().item() and (bucket[32 + w.numel():] == 3).all().item()
    w2 = ops_data["ws"][1].clone().requires_grad_(True)
    linear(ops_data["x"], w2).backward(ops_data["dys"][1])
    assert torch.equal(w.grad, w2.grad)


def _llama_run(monkeypatch, mode, state, tokens, targets, cfg, dtype):
    from distributeddataparallel_amd.models.llama import llama_tiny

    monkeypatch.setenv("XDDP_FP8", "0" if mode == "fp32" else mode)
    monkeypatch.setenv("XDDP_FUSED_TRANSFORMER", "0" if mode == "fp32" else "1")
    model = llama_tiny(**cfg)
    model.load_state_dict(state)
    model = model.cuda().to(dtype)
    logits = model(tokens)
    loss = F.cross_entropy(logits.float().view(-1, logits.shape[-1]), targets.view(-1))
    loss.backward()
    L0 = model.layers[0]
    return dict(loss=loss.detach().float(), wq=L0.attention.wq.weight.grad.float(), w1=L0.feed_forward.w1.weight.grad.float(),
                emb=model.tok_embeddings.weight.grad.float())


def test_llama_tiny_fp8(monkeypatch):
    """Two-layer Llama (dim 256, ffn 512, vocab 512, S = 128), loss + backward, against the fp32
    reference ops. The kernel path's error on the loss and on the wq / w1 / embedding gradients
    is at most 1.25 x the emulation's (25 % for uncorrelated rounding flips); the FP8 GEMM ran
    3 x 7 x layers times, so the LM head did not use it. Measured on one MI355X (kernel / emulation
    error): loss 8.2e-4 / 2.5e-3, wq 0.1418 / 0.1412, w1 0.1228 / 0.1215, embeddings 0.1396 / 0.1390."""
    from distributeddataparallel_amd._native import load
    from distributeddataparallel_amd.models.llama import llama_tiny

    cfg = dict(dim=256, n_heads=4, n_kv_heads=2, ffn_dim=512, vocab_size=512, max_seq_len=128)
    torch.manual_seed(0)
    state = llama_tiny(**cfg).state_dict()
    g = torch.Generator().manual_seed(3)
    tokens = torch.randint(0, 512, (1, 128), generator=g).cuda()
    targets = torch.randint(0, 512, (1, 128), generator=g).cuda()
    ref = _llama_run(monkeypatch, "fp32", state, tokens, targets, cfg, torch.float32)
    emu = _llama_run(monkeypatch, "emulate", state, tokens, targets, cfg, torch.bfloat16)

    C = load()
    calls, orig = [], C.gemm_fp8_nt
    monkeypatch.setattr(C, "gemm_fp8_nt", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    ker = _llama_run(monkeypatch, "1", state, tokens, targets, cfg, torch.bfloat16)
    assert len(calls) == 3 * 7 * 2, len(calls)

    def err(run, k):
        return abs((run[k] - ref[k]).item()) if k == "loss" else _rel(run[k], ref[k])

    ratios = {}
    for k in ("loss", "wq", "w1", "emb"):
        ek, ee = err(ker, k), err(emu, k)
        ratios[k] = ek / max(ee, 1e-12)
        print(f"llama_tiny fp8 {k}: kernel err {ek:.4e} emulate err {ee:.4e} ratio {ratios[k]:.3f}")
    assert torch.isfinite(ker["loss"]).item()
    for k, r in ratios.items():
        assert r <= 1.25, (k, r)
