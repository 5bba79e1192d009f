"""CPU-only checks of modeling/grad_ops.py: the stacked operand of two layers (the RPN head's and the predictor's shapes), the
operand cache and the modules that keep their re-laid weights in one (rebuilt after an optimizer step on any keyed parameter), and
the flipped weight of the 3x3 dgrad against autograd.  No kernel is launched here."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from layoutdit_amd import config as cfgs
from layoutdit_amd.modeling import DiTWithFPN, LayoutDetectionModel, RPNHead
from layoutdit_amd.modeling.grad_ops import OperandCache, ParamCache, flip_ihwo, param_key, stack_rows
from layoutdit_amd.modeling.roi_heads import FastRCNNPredictor, TwoMLPHead


def _sgd_step(p):
    """An in-place update as an optimizer makes it (moves the parameter's version counter)."""
    p.grad = torch.ones_like(p)
    torch.optim.SGD([p], lr=1.0).step()
    p.grad = None


@pytest.mark.parametrize("n0,n1,K,multiple,rows", [(3, 12, 256, 4, 16), (6, 24, 1024, 32, 32)])     # RPN head A = 3; predictor NC = 6
def test_stack_rows_places_the_layers_and_zeroes_the_padding(n0, n1, K, multiple, rows):
    g = torch.Generator().manual_seed(n0)
    w0, w1 = nn.Parameter(torch.randn(n0, K, generator=g)), nn.Parameter(torch.randn(n1, K, generator=g))
    b0, b1 = nn.Parameter(torch.randn(n0, generator=g)), nn.Parameter(torch.randn(n1, generator=g))
    w, b = stack_rows((w0, w1), (b0, b1), multiple)
    assert tuple(w.shape) == (rows, K) and tuple(b.shape) == (rows,)
    assert w.dtype == b.dtype == torch.float32 and w.is_contiguous() and b.is_contiguous() and not w.requires_grad and not b.requires_grad
    assert torch.equal(w[:n0], w0) and torch.equal(w[n0:n0 + n1], w1) and torch.equal(b[:n0], b0) and torch.equal(b[n0:n0 + n1], b1)
    assert rows > n0 + n1 and not w[n0 + n1:].any() and not b[n0 + n1:].any()


def test_param_cache_keeps_its_value_until_the_key_changes():
    p, q = nn.Parameter(torch.zeros(3)), nn.Parameter(torch.zeros(2))
    cache, builds = ParamCache(), []

    def build():
        builds.append(1)
        return torch.cat([p.detach(), q.detach()])
    first = cache.get(param_key(p, q), build)
    assert cache.get(param_key(p, q), build) is first and len(builds) == 1
    for i, t in enumerate((p, q)):                                                  # any keyed parameter
        _sgd_step(t)
        again = cache.get(param_key(p, q), build)
        assert again is not first and len(builds) == 2 + i and torch.equal(again, torch.cat([p.detach(), q.detach()]))
        assert cache.get(param_key(p, q), build) is again
    assert cache.get((param_key(p, q), 7), build) is not again and len(builds) == 4  # whatever else the key carries
    cache.clear()
    assert cache.value is None and cache.get(param_key(p, q), build) is not None and len(builds) == 5


def test_operand_cache_keeps_an_entry_until_its_key_changes():
    p, q = nn.Parameter(torch.zeros(3)), nn.Parameter(torch.zeros(2))
    cache, builds = OperandCache(), []

    def build():
        builds.append(1)
        return torch.cat([p.detach(), q.detach()])
    assert not cache.filled() and not cache.filled("pq")
    first = cache.get("pq", (p, q), build)
    assert cache.get("pq", (p, q), build) is first and len(builds) == 1 and cache.filled() and cache.filled("pq")
    for i, t in enumerate((p, q)):                                                  # any keyed parameter
        _sgd_step(t)
        again = cache.get("pq", (p, q), build)
        assert again is not first and len(builds) == 2 + i and torch.equal(again, torch.cat([p.detach(), q.detach()]))
        assert cache.get("pq", (p, q), build) is again
    assert cache.get("pq", (p, q), build, 7) is not again and len(builds) == 4      # whatever else the key carries
    cache.clear()
    assert not cache.filled("pq") and cache.get("pq", (p, q), build) is not None and len(builds) == 5


def test_operand_cache_rebuilds_an_entry_alone_and_clear_empties_all():
    p, q = nn.Parameter(torch.zeros(3)), nn.Parameter(torch.zeros(2))
    cache, builds = OperandCache(), []

    def builder(name, t):
        def build():
            builds.append(name)
            return t.detach().clone()
        return build
    got = {"p": cache.get("p", (p,), builder("p", p)), ("q", 0): cache.get(("q", 0), (q,), builder("q", q), 5)}
    assert builds == ["p", "q"] and cache.filled("p") and cache.filled(("q", 0)) and not cache.filled("q")
    _sgd_step(p)                                                                    # p's key alone moves
    assert cache.get(("q", 0), (q,), builder("q", q), 5) is got[("q", 0)] and builds == ["p", "q"]
    new_p = cache.get("p", (p,), builder("p", p))
    assert new_p is not got["p"] and torch.equal(new_p, p.detach()) and builds == ["p", "q", "p"]
    assert cache.get(("q", 0), (q,), builder("q", q), 5) is got[("q", 0)]           # the other entry keeps its object
    assert cache.get(("q", 0), (q,), builder("q", q), 6) is not got[("q", 0)] and cache.get("p", (p,), builder("p", p)) is new_p
    cache.clear()
    assert not cache.filled() and not cache.filled("p") and not cache.filled(("q", 0))


def test_every_stage_keeps_one_cache_that_the_invalidating_loop_finds():
    """``DetectorTrainStep`` has no CPU path, so this walks the modules as its ``invalidate_caches`` does: by the one attribute and its
    type, without naming a stage class."""
    torch.manual_seed(0)
    model = LayoutDetectionModel(config=cfgs.vit_micro())
    m = model.model
    stages = (m.backbone, m.rpn.head, m.roi_heads.box_head, m.roi_heads.box_predictor)
    assert [type(s) for s in stages] == [DiTWithFPN, RPNHead, TwoMLPHead, FastRCNNPredictor]
    assert all(isinstance(s._operand_cache, OperandCache) for s in stages)
    assert len({id(s._operand_cache) for s in stages}) == 4                         # one each
    owners = [mod for mod in model.modules() if isinstance(getattr(mod, "_operand_cache", None), OperandCache)]
    assert len(owners) == 4 and all(any(o is s for s in stages) for o in owners)
    for s in stages:                                                                # and no second cache under another name
        assert [k for k, v in vars(s).items() if isinstance(v, OperandCache)] == ["_operand_cache"]
    for i in range(4):
        m.backbone._ohwi(i)
    m.rpn.head._operands(), m.roi_heads.box_head.fc6_weight_hwc(256, 7, 7), m.roi_heads.box_predictor._operands()
    assert all(s._operand_cache.filled() for s in stages)
    for mod in model.modules():
        cache = getattr(mod, "_operand_cache", None)
        if isinstance(cache, OperandCache):
            cache.clear()
    assert not any(s._operand_cache.filled() for s in stages)


def test_rpn_head_operands_follow_every_parameter():
    torch.manual_seed(0)
    head = RPNHead(256, 3)

    def want():
        w1 = torch.zeros(16, 256)
        w1[:3], w1[3:15] = head.cls_logits.weight.detach().view(3, 256), head.bbox_pred.weight.detach().view(12, 256)
        b1 = torch.zeros(16)
        b1[:3], b1[3:15] = head.cls_logits.bias.detach(), head.bbox_pred.bias.detach()
        return head.conv[0][0].weight.detach().permute(0, 2, 3, 1), head.conv[0][0].bias.detach(), w1, b1
    ops0 = head._operands()
    assert all(a is b for a, b in zip(head._operands(), ops0))
    assert tuple(ops0[2].shape) == (16, 256) and ops0[0].is_contiguous() and all(torch.equal(a, b) for a, b in zip(ops0, want()))
    for p in head.parameters():
        before = head._operands()
        old = [t.clone() for t in before]                                           # (the 3x3's bias is a view of its parameter)
        _sgd_step(p)
        after = head._operands()
        assert after[2] is not before[2] and all(torch.equal(a, b) for a, b in zip(after, want())), tuple(p.shape)
        assert not all(torch.equal(a, b) for a, b in zip(after, old))
        assert all(a is b for a, b in zip(head._operands(), after))


def test_fpn_ohwi_follows_its_level_alone():
    torch.manual_seed(0)
    m = DiTWithFPN(config=cfgs.vit_micro())
    first = [m._ohwi(i) for i in range(4)]
    assert all(m._ohwi(i) is first[i] for i in range(4))
    for i in range(4):
        w = m.fpn.layer_blocks[i][0].weight
        _sgd_step(w)
        now = m._ohwi(i)
        assert now is not first[i] and now.is_contiguous() and torch.equal(now, w.detach().permute(0, 2, 3, 1))
        assert not torch.equal(now, first[i]) and m._ohwi(i) is now
        assert all(m._ohwi(j) is first[j] for j in range(i + 1, 4))               # the other levels' operands stay


def test_flip_ihwo_is_the_dgrad_weight():
    """Unequal channels and sides: a swapped axis cannot pass.  Small integers in float64: every sum is exact in any order."""
    B, Cin, Cout, H, W = 1, 2, 3, 3, 4
    g = torch.Generator().manual_seed(1)
    x = torch.randint(-4, 5, (B, Cin, H, W), generator=g).double().requires_grad_(True)
    w = torch.randint(-4, 5, (Cout, Cin, 3, 3), generator=g).double()
    dy = torch.randint(-4, 5, (B, Cout, H, W), generator=g).double()
    (F.conv2d(x, w, padding=1) * dy).sum().backward()
    wf = flip_ihwo(w)
    assert tuple(wf.shape) == (Cin, 3, 3, Cout) and wf.is_contiguous()
    assert torch.equal(F.conv2d(dy, wf.permute(0, 3, 1, 2), padding=1), x.grad)
