"""``FusedAdafactor`` without a GPU: its torch path against ``torch.optim.Adafactor``, state dicts both
ways, and the refusals. The bound is the fp32 bound of tests/_af_refs.py."""
import copy

import pytest
import torch

from distributeddataparallel_amd.optim import FusedAdafactor
from _af_refs import close

SHAPES = [(33, 70), (3, 5, 9), (17,)]
KW = dict(lr=1e-2, weight_decay=0.1, d=1.0)


def params(seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(0.05 * torch.randn(s, generator=gen)) for s in SHAPES]


def steps(opts, lists, n, seed):
    gen = torch.Generator().manual_seed(seed)
    for _ in range(n):
        for ps in zip(*lists):
            g = torch.randn(ps[0].shape, generator=gen)
            for p in ps:
                p.grad = g.clone()
        for opt in opts:
            opt.step()


def same(a, b, oa, ob):
    for p, q in zip(a, b):
        close(p.detach(), q.detach().double(), "w", f"param {tuple(p.shape)}")
        for k in ("row_var", "col_var", "variance"):
            assert (k in oa.state[p]) == (k in ob.state[q])
            if k in oa.state[p]:
                close(oa.state[p][k], ob.state[q][k].double(), k, k)
                assert oa.state[p][k].shape == ob.state[q][k].shape and oa.state[p][k].dtype == torch.float32


def test_five_steps_follow_torch():
    a, b = params(), params()
    oa, ob = FusedAdafactor(a, **KW), torch.optim.Adafactor(b, foreach=False, **KW)
    steps([oa, ob], [a, b], 5, 1)
    same(a, b, oa, ob)
    assert oa.state[a[0]]["step"] == 5 and not hasattr(oa, "advance") and not hasattr(oa, "step_slices")


@pytest.mark.parametrize("ours_first", [True, False])
def test_state_dict_round_trip_with_torch(ours_first):
    a, b = params(), params()
    oa, ob = FusedAdafactor(a, **KW), torch.optim.Adafactor(b, foreach=False, **KW)
    src, src_params = (oa, a) if ours_first else (ob, b)
    steps([src], [src_params], 2, 2)
    c = [torch.nn.Parameter(p.detach().clone()) for p in src_params]
    oc = torch.optim.Adafactor(c, foreach=False, **KW) if ours_first else FusedAdafactor(c, **KW)
    oc.load_state_dict(copy.deepcopy(src.state_dict()))  # (a state dict holds the live state tensors)
    steps([src, oc], [src_params, c], 2, 3)
    same(*((src_params, c, src, oc) if ours_first else (c, src_params, oc, src)))


@pytest.mark.parametrize("kw", [dict(lr=-1.0), dict(beta2_decay=0.1), dict(eps=(-1.0, 1e-3)), dict(eps=(None, -1.0)),
                                dict(d=0.5), dict(weight_decay=-0.1)])
def test_bad_arguments_are_refused_as_by_torch(kw):
    for cls in (FusedAdafactor, torch.optim.Adafactor):
        with pytest.raises(ValueError):
            cls(params(), **kw)


def test_fp64_and_the_tail_schedule_are_refused():
    from distributeddataparallel_amd.parallel.distributed import DistributedDataParallel as DDP

    p = torch.nn.Parameter(torch.zeros(4, 4, dtype=torch.float64))
    p.grad = torch.ones_like(p)
    opt = FusedAdafactor([p])
    with pytest.raises(TypeError, match="fp64"):
        opt.step()
    assert len(opt.state[p]) == 0
    with pytest.raises(TypeError, match="schedule='backward'"):
        DDP.register_overlapped_optimizer(object(), opt, schedule="tail")
