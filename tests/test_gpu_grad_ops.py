"""modeling/grad_ops.py on the GPU: ``conv3x3_bwd`` and ``linear_bwd`` called directly, against float64 torch autograd, and the RPN
head's differentiable level on the head's cached operands.  Gates: those of tests/test_gpu_fpn.py's building blocks (dgrad 1e-5, the
bf16 wgrad 1e-5 against the operands it multiplies and 1e-2 against the fp32 problem, bias 1e-6) and of
test_heads_backward_matches_float64_autograd (input and bias gradients 2e-5, the bf16-operand weight gradient 3e-2)."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import torch.nn.functional as F                      # noqa: E402

from layoutdit_amd import synth                       # noqa: E402
from layoutdit_amd.modeling import RPNHead            # noqa: E402
from layoutdit_amd.modeling.grad_ops import conv3x3_bwd, linear_bwd    # noqa: E402
from tests.util import rel_l2                         # noqa: E402

DEV = "cuda:0"
BF = torch.bfloat16


def _rand(seed, *shape, scale=1.0):
    return torch.from_numpy((scale * synth.normal(seed, 9, int(np.prod(shape)))).astype(np.float32).reshape(shape))


def _one_off(outs_all, fn):
    """Every call with exactly one ``need_*`` false: that output is None, the others have the bits of the call that wants all three."""
    for need in itertools.product((True, False), repeat=3):
        if sum(need) != 2:
            continue
        for want, full, got in zip(need, outs_all, fn(*need)):
            assert (got is None) if not want else torch.equal(got, full), need


# (1, 1, 1, 32, 32): every tap but the centre reads only padding, the slack rows are most of the operand; (3, 5, 9, 64, 96): Cin != Cout
# and H != W, so a transposed weight gradient or a wrong row pitch cannot pass
@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 6, 9, 64, 64), (1, 1, 1, 32, 32), (3, 5, 9, 64, 96)])
def test_conv3x3_bwd_matches_float64_autograd(B, H, W, Cin, Cout):
    x, dy, wt = _rand(50, B, H, W, Cin), _rand(51, B, H, W, Cout), _rand(52, Cout, Cin, 3, 3, scale=0.05)
    xd, dyd, wd = x.to(DEV), dy.to(DEV), wt.to(DEV)
    dx, dw, db = outs = conv3x3_bwd(dyd, xd, wd, True, True, True)
    assert tuple(dx.shape) == (B, H, W, Cin) and tuple(dw.shape) == (Cout, Cin, 3, 3) and tuple(db.shape) == (Cout,)
    xr, wr = x.double().permute(0, 3, 1, 2).requires_grad_(True), wt.double().requires_grad_(True)
    (F.conv2d(xr, wr, padding=1) * dy.double().permute(0, 3, 1, 2)).sum().backward()
    wr2 = wt.double().requires_grad_(True)                        # the wgrad of the bf16-rounded operands it actually multiplies
    (F.conv2d(x.to(BF).double().permute(0, 3, 1, 2), wr2, padding=1) * dy.to(BF).double().permute(0, 3, 1, 2)).sum().backward()
    errs = (rel_l2(dx.cpu().numpy(), xr.grad.permute(0, 2, 3, 1).numpy()), rel_l2(dw.cpu().numpy(), wr2.grad.numpy()),
            rel_l2(dw.cpu().numpy(), wr.grad.numpy()), rel_l2(db.cpu().numpy(), dy.double().reshape(-1, Cout).sum(0).numpy()))
    print("dgrad %.3e, wgrad on rounded operands %.3e, wgrad %.3e, bias %.3e" % errs)
    assert errs[0] < 1e-5 and errs[1] < 1e-5 and errs[2] < 1e-2 and errs[3] < 1e-6
    _one_off(outs, lambda nx, nw, nb: conv3x3_bwd(dyd, xd, wd, nx, nw, nb))


def _linear_errs(outs, dy, x, w):
    g_x, g_w, g_b = (t.cpu().numpy() for t in outs)
    dy64, n = dy.double(), w.shape[0]
    return (rel_l2(g_x, (dy64[:, :n] @ w.double()).numpy()), rel_l2(g_w, (dy64.T @ x.double()).numpy()), rel_l2(g_b, dy64.sum(0).numpy()))


@pytest.mark.parametrize("M,N,K", [(74, 32, 64), (32, 32, 1024)])
def test_linear_bwd_matches_float64_autograd(M, N, K):
    dy, x, w = _rand(60, M, N), _rand(61, M, K), _rand(62, N, K, scale=0.1)
    dyd, xd, wd = dy.to(DEV), x.to(DEV), w.to(DEV)
    outs = linear_bwd(dyd, xd, wd, True, True, True)
    assert [tuple(t.shape) for t in outs] == [(M, K), (N, K), (N,)]
    errs = _linear_errs(outs, dy, x, w)
    print("input %.3e, weight %.3e, bias %.3e" % errs)
    assert errs[0] < 2e-5 and errs[1] < 3e-2 and errs[2] < 2e-5
    _one_off(outs, lambda nx, nw, nb: linear_bwd(dyd, xd, wd, nx, nw, nb))


def test_linear_bwd_zero_extends_a_stacked_weight():
    """The RPN head's form: 15 live columns of 32 against the 16-row stacked weight - the bits of the call on the weight padded to
    32 rows by hand."""
    M, N, rows, Cc = 45, 32, 16, 256
    dy, x, w = _rand(63, M, N), _rand(64, M, Cc), _rand(65, rows, Cc, scale=0.1)
    dy[:, 15:], w[15:] = 0.0, 0.0
    w32 = torch.zeros(N, Cc)
    w32[:rows] = w
    outs = linear_bwd(dy.to(DEV), x.to(DEV), w.to(DEV), True, True, True)
    assert [tuple(t.shape) for t in outs] == [(M, Cc), (N, Cc), (N,)]
    for got, want in zip(outs, linear_bwd(dy.to(DEV), x.to(DEV), w32.to(DEV), True, True, True)):
        assert torch.equal(got, want)
    errs = _linear_errs(outs, dy, x, w)
    assert errs[0] < 2e-5 and errs[1] < 3e-2 and errs[2] < 2e-5 and not outs[1][15:].any() and not outs[2][15:].any()


def test_rpn_head_level_reads_the_cached_operands_of_the_current_weights():
    """Two forward_level + backward passes with an optimizer step between them: the second pass runs on the updated weights - the
    bits of a freshly constructed head loaded with the same state_dict."""
    torch.manual_seed(0)
    head = RPNHead(64, 3).to(DEV).train()
    x = _rand(66, 2, 64, 5, 7).to(DEV)
    opt = torch.optim.SGD(head.parameters(), lr=0.5)

    def one_pass(h):
        logits, deltas = h.forward_level(x)
        assert logits.requires_grad and tuple(logits.shape) == (2, 5 * 7 * 3) and tuple(deltas.shape) == (2, 5 * 7 * 3, 4)
        (logits.sum() + deltas.sum()).backward()
        return logits.detach().clone(), deltas.detach().clone()
    first = one_pass(head)
    assert all(p.grad is not None and bool(p.grad.any()) for p in head.parameters())
    opt.step()
    second = one_pass(head)
    fresh = RPNHead(64, 3).to(DEV).train()
    fresh.load_state_dict(head.state_dict())
    want = one_pass(fresh)
    assert not torch.equal(second[0], first[0]) and not torch.equal(second[1], first[1])
    assert torch.equal(second[0], want[0]) and torch.equal(second[1], want[1])
    with torch.no_grad():                                         # the eval path reads the same operands
        assert torch.equal(head.eval().forward_level(x)[0], second[0])


def _masked(seed, *shape, dtype=torch.float32):
    """``dy``, a ReLU output ``act`` of that shape (about half of it zero, element [0, .., 0] among them) and ``dy`` with one NaN at
    that masked position."""
    dy, act = _rand(seed, *shape).to(DEV), torch.relu(_rand(seed + 1, *shape)).to(DEV).to(dtype)
    act.view(-1)[0] = 0
    poisoned = dy.clone()
    poisoned.view(-1)[0] = float("nan")
    return dy, act, poisoned


# the smallest shapes that reach the fp32 arm with a mask: N = 32 is below the bf16 GEMM's k-tile (fp32 arm under either grad_dtype);
# N = 64 with a bf16 act is the box head under train_dtype="bf16", grad_dtype="f32"
@pytest.mark.parametrize("N,grad_dtype,act_dtype", [(32, "f32", torch.float32), (32, "bf16", torch.float32), (64, "f32", BF)])
def test_linear_bwd_fp32_arm_masks_by_multiplication(N, grad_dtype, act_dtype):
    M, K = 3, 64
    dy, act, poisoned = _masked(70, M, N, dtype=act_dtype)
    x, w = _rand(72, M, K).to(DEV), _rand(73, N, K, scale=0.1).to(DEV)
    got = linear_bwd(dy, x, w, True, True, True, grad_dtype, act=act)
    want = linear_bwd(dy * (act > 0), x, w, True, True, True, grad_dtype)
    assert all(torch.equal(g, t) for g, t in zip(got, want))
    g_b = linear_bwd(poisoned, x, w, True, True, True, grad_dtype, act=act)[2]
    assert not bool(torch.isfinite(g_b).all())                    # NaN * 0: what the default configuration has always given
    if N == 64:                                                   # the fused launch of the bf16 arm selects: the same input stays finite
        assert all(bool(torch.isfinite(t).all()) for t in linear_bwd(poisoned, x, w, True, True, True, "bf16", act=act))


@pytest.mark.parametrize("grad_dtype", ["f32", "bf16"])
def test_conv3x3_bwd_fp32_arm_masks_by_multiplication(grad_dtype):
    B, h, w, Cout, Cin = 1, 2, 3, 32, 64                          # Cout = 32: below the k-tile, the fp32 arm under either grad_dtype
    dy, act, poisoned = _masked(74, B, h, w, Cout)
    x, wt = _rand(76, B, h, w, Cin).to(DEV), _rand(77, Cout, Cin, 3, 3, scale=0.05).to(DEV)
    got = conv3x3_bwd(dy, x, wt, True, True, True, grad_dtype, act=act.view(B * h * w, Cout))      # the stages hand the pixel rows
    want = conv3x3_bwd(dy * (act > 0), x, wt, True, True, True, grad_dtype)
    assert all(torch.equal(g, t) for g, t in zip(got, want))
    assert not bool(torch.isfinite(conv3x3_bwd(poisoned, x, wt, True, True, True, grad_dtype, act=act)[2]).all())
