"""The label-smoothed cross-entropy kernels with top-1 / top-k counts (csrc/kernels/loss.hip) on the GPU,
against the float64 oracles and under the bounds of tests/test_loss_metrics.py (those of
tests/test_gpu_kernels.py::test_xent_vs_torch). Counts must equal the oracle exactly.

Shapes: (3, 10) scalar path with 54 empty lanes; (4, 8) one bf16 vector, 63 empty lanes; (5, 1000) aligned
rows with an uneven number of 16-byte vectors per lane (125 or 250 over 64 lanes); (129, 4097) an odd pitch,
so every row is misaligned, and more than one block; (256, 1000) the training shape. A view one element past
a 16-byte boundary takes the scalar path at an aligned pitch; logits of randn * 30 overflow exp without the
running max.
"""
import functools

import pytest
import torch

from test_loss_metrics import GRAD_TOL, check_against_oracle, edge_case_counts, make_case

pytestmark = pytest.mark.gpu

SHAPES = [(3, 10), (4, 8), (5, 1000), (129, 4097), (256, 1000)]
DTYPES = [torch.float32, torch.bfloat16]


@functools.lru_cache(maxsize=None)
def _case(B, C, dtype, seed=0, scale=3.0):
    return make_case(B, C, dtype, seed, scale)  # shared, never written to


@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,C", SHAPES)
def test_matches_oracles(cuda, B, C, dtype, eps, k):
    x, y = _case(B, C, dtype)
    check_against_oracle(x.to(cuda), y.to(cuda), eps, k, dtype, strict=B >= 20)


@pytest.mark.parametrize("dtype", DTYPES)
def test_view_off_alignment(cuda, dtype):
    B, C = 64, 1000
    x, y = _case(B, C, dtype, seed=1)
    view = torch.empty(B * C + 1, device=cuda, dtype=dtype)[1:].view(B, C)
    view.copy_(x)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    loss, stats, grad = check_against_oracle(view, y.to(cuda), 0.1, 5, dtype)
    # the vector path on an aligned copy of the same values counts the same and agrees within the bounds
    loss2, stats2, grad2 = check_against_oracle(x.to(cuda), y.to(cuda), 0.1, 5, dtype)
    assert torch.equal(stats[1:], stats2[1:])
    torch.testing.assert_close(grad.float(), grad2.float(), **GRAD_TOL[dtype])


def test_large_logits_need_the_running_max(cuda):
    x, y = _case(64, 1000, torch.float32, seed=2, scale=30.0)
    assert float(x.max()) > 100.0  # exp overflows fp32 above 88.7
    loss, _, grad = check_against_oracle(x.to(cuda), y.to(cuda), 0.1, 5, torch.float32)
    assert torch.isfinite(loss) and torch.isfinite(grad).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_cases(cuda, dtype):
    edge_case_counts(cuda, dtype)


def test_minus_inf_logits(cuda):
    """Masked classes: -inf logits add nothing, also where a whole lane or vector holds nothing else."""
    from distributed_learning_amd.ops import cross_entropy, cross_entropy_with_metrics

    x, y = _case(5, 1000, torch.float32)
    x = x.clone()
    x[:, 8:] = float("-inf")  # lanes 1.. of the vector path, lanes 8.. of the scalar one see only -inf
    y = y % 8
    for xs in (x.to(cuda), x[:, :999].contiguous().to(cuda)):
        loss, stats = cross_entropy_with_metrics(xs, y.to(cuda), 0.0, 5)
        ref = torch.nn.functional.cross_entropy(xs.double().cpu(), y)
        torch.testing.assert_close(loss.double().cpu(), ref, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(cross_entropy(xs, y.to(cuda)).double().cpu(), ref, rtol=1e-5, atol=1e-5)
        assert float(stats[1]) == 5.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_bitwise_reproducible_and_zero_eps_matches_plain_loss(cuda, dtype):
    from distributed_learning_amd.ops import cross_entropy, cross_entropy_with_metrics

    x, y = _case(256, 1000, dtype)
    y = y.to(cuda)
    runs = []
    for _ in range(2):
        xr = x.to(cuda).requires_grad_(True)
        loss, stats = cross_entropy_with_metrics(xr, y, 0.1, 5)
        loss.backward()
        runs.append((loss.detach(), stats, xr.grad))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    xa, xb = x.to(cuda).requires_grad_(True), x.to(cuda).requires_grad_(True)
    la = cross_entropy_with_metrics(xa, y, 0.0, 5)[0]
    lb = cross_entropy(xb, y)
    la.backward()
    lb.backward()
    torch.testing.assert_close(la.detach(), lb.detach(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(xa.grad.float(), xb.grad.float(), **GRAD_TOL[dtype])


def test_binding_checks(cuda):
    from distributed_learning_amd.ops import _ext

    C = _ext.require()
    x = torch.zeros(4, 10, device=cuda)
    y = torch.zeros(4, dtype=torch.long, device=cuda)
    stats, ws = C.xent_metrics_fwd(x, y, 0.0, 1)
    assert stats.shape == (4,) and ws.shape == (17,) and float(ws[-1]) == float(stats[0] / stats[1])
    for bad in (lambda: C.xent_metrics_fwd(x, y, 1.0, 1), lambda: C.xent_metrics_fwd(x, y, -0.5, 1),
                lambda: C.xent_metrics_fwd(x, y, 0.0, 0), lambda: C.xent_metrics_fwd(x, y[:3], 0.0, 1),
                lambda: C.xent_metrics_fwd(x.cpu(), y, 0.0, 1), lambda: C.xent_metrics_fwd(x.half(), y, 0.0, 1),
                lambda: C.xent_metrics_fwd(x.t(), y, 0.0, 1), lambda: C.xent_metrics_fwd(x, y.int(), 0.0, 1),
                lambda: C.xent_smooth_bwd(x, y, ws[:5], stats, stats[:1], 0.0),
                lambda: C.xent_smooth_bwd(x, y, ws, stats, stats[:1], 1.0)):
        with pytest.raises(RuntimeError):
            bad()


def test_graph_capture_replays_to_the_eager_result(cuda):
    from distributed_learning_amd.ops import cross_entropy_with_metrics
    from distributed_learning_amd.parallel.graphs import GraphedStep

    feeds = [_case(256, 1000, torch.bfloat16, seed=s) for s in (10, 11, 12)]
    xs = feeds[0][0].to(cuda).requires_grad_(True)  # the static buffers the graph reads
    ys = feeds[0][1].to(cuda)

    def step():
        xs.grad = None
        loss, stats = cross_entropy_with_metrics(xs, ys, 0.1, 5)
        loss.backward()
        return loss.detach(), stats, xs.grad

    runner = GraphedStep(step, warmup=2, device=cuda)
    for x, y in feeds:
        with torch.no_grad():
            xs.copy_(x)
            ys.copy_(y)
        loss, stats, grad = runner()
        xe = x.to(cuda).requires_grad_(True)
        le, se = cross_entropy_with_metrics(xe, y.to(cuda), 0.1, 5)
        le.backward()
        assert torch.equal(loss, le.detach()) and torch.equal(stats, se) and torch.equal(grad, xe.grad)
    assert runner.captured and runner.calls == 3
