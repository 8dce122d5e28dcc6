"""Every op bound in csrc/nn_bindings.cpp that takes a tensor refuses host tensors with a RuntimeError and
returns normally to Python (CPU: the argument checks are host code and run before any launch). The arguments are
well-formed apart from living in host memory, so it is the device check that speaks."""
import os
import re

import pytest
import torch

from distributed_learning_amd.ops import _ext

pytestmark = pytest.mark.skipif(not _ext.available(), reason="native extension not built")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, C, H, W = 2, 16, 4, 4
M = N * H * W
BF, F32 = torch.bfloat16, torch.float32


def act(c=C, h=H, w=W, dtype=BF):
    return torch.zeros(N, c, h, w, dtype=dtype).contiguous(memory_format=torch.channels_last)


def mat(r=M, c=C):
    return torch.zeros(r, c, dtype=BF)


def vec(n=C):
    return torch.ones(n)


def ws(c=C):
    return torch.zeros(7 * c)


def bits(elems=M * C):
    return torch.zeros((elems + 7) // 8, dtype=torch.uint8)


def parts(rows=1, c=C):
    return torch.zeros(rows, c, 2)


def pos(c=C, h=H // 2, w=W // 2):
    return torch.zeros(N, c, h, w, dtype=torch.uint8).contiguous(memory_format=torch.channels_last)


def w3(co=64, ci=64):
    return torch.zeros(co, ci, 3, 3, dtype=BF).contiguous(memory_format=torch.channels_last)


# op -> a call with host tensors only
CALLS = {
    "bn_act_fwd": lambda C_: C_.bn_act_fwd(act(), None, vec(), vec(), vec(), vec(), True, 0.1, 1e-5, True),
    "bn_act_bwd": lambda C_: C_.bn_act_bwd(act(), None, None, act(), ws(), vec(), 1, False),
    "bn_dual_fwd": lambda C_: C_.bn_dual_fwd(act(), act(), vec(), vec(), vec(), vec(), vec(), vec(), vec(), vec(), 0.1,
                                             0.1, 1e-5, 1e-5, True, None, None),
    "bn_dual_bwd": lambda C_: C_.bn_dual_bwd(act(), bits(), act(), ws(), vec(), act(), ws(), vec()),
    "bn_apply_deferred": lambda C_: C_.bn_apply_deferred(act(), act(), ws(), None, act(), bits()),
    "bn_concat_fwd": lambda C_: C_.bn_concat_fwd([act()], [vec()], [vec()], [vec()], [vec()], [0.1], [1e-5], [parts()],
                                                 act()),
    "bn_concat_bwd": lambda C_: C_.bn_concat_bwd(act(), [act()], [vec()], [ws()]),
    "bn_group_fwd": lambda C_: C_.bn_group_fwd([act()], [vec()], [vec()], [vec()], [vec()], [0.1], [1e-5], [parts()]),
    "bn_group_bwd": lambda C_: C_.bn_group_bwd([act()], [act()], [vec()], [ws()]),
    "bn_relu_maxpool_fwd": lambda C_: C_.bn_relu_maxpool_fwd(act(), vec(), vec(), vec(), vec(), 0.1, 1e-5, 3, 2, 1),
    "bn_relu_maxpool_bwd": lambda C_: C_.bn_relu_maxpool_bwd(act(h=H // 2, w=W // 2), pos(), act(), ws(), vec(), 3, 2, 1),
    "maxpool_fwd": lambda C_: C_.maxpool_fwd(act(), 3, 2, 1),
    "maxpool_bwd": lambda C_: C_.maxpool_bwd(act(h=H // 2, w=W // 2), pos(), H, W, 3, 2, 1),
    "gap_fwd": lambda C_: C_.gap_fwd(act()),
    "gap_bwd": lambda C_: C_.gap_bwd(torch.zeros(N, C, dtype=BF), H, W),
    "subsample2": lambda C_: C_.subsample2(act()),
    "gemm_nt": lambda C_: C_.gemm_nt(mat(), mat(64, C)),
    "gemm_nt_bn": lambda C_: C_.gemm_nt_bn(mat(), mat(C, 64), None, True, mat(M, 64), ws(64), None, 1),
    "gemm_nt_apply": lambda C_: C_.gemm_nt_apply(mat(M, 64), mat(M, 64), ws(64), None, mat(64, 64), True, mat(M, 64),
                                                 bits(M * 64)),
    "gemm_nt_stream_apply": lambda C_: C_.gemm_nt_stream_apply(mat(M, 64), ws(64), mat(64, 64), mat(M, 64)),
    "gemm_tn": lambda C_: C_.gemm_tn(mat(), mat()),
    "conv1x1_dual": lambda C_: C_.conv1x1_dual(mat(M, 64), mat(), mat(64, C)),
    "conv3x3_fwd": lambda C_: C_.conv3x3_fwd(act(64), w3()),
    "conv3x3_dgrad": lambda C_: C_.conv3x3_dgrad(act(64), w3()),
    "conv3x3s2_dgrad": lambda C_: C_.conv3x3s2_dgrad(act(64), w3(), 2 * H, 2 * W),
    "conv3x3_dgrad_bn": lambda C_: C_.conv3x3_dgrad_bn(act(64), w3(), None, act(64), ws(64), None, 1),
    "conv3x3_wgrad": lambda C_: C_.conv3x3_wgrad(act(64), act(64)),
    "conv_f32_fwd": lambda C_: C_.conv_f32_fwd(act(dtype=F32), torch.zeros(C, 3, 3, C), 1),
    "conv_f32_wgrad": lambda C_: C_.conv_f32_wgrad(act(dtype=F32), act(dtype=F32), 3, 3, 1),
    "stem_fwd": lambda C_: C_.stem_fwd(act(3, 8, 8), torch.zeros(64, 256, dtype=BF), True),
    "stem_wgrad": lambda C_: C_.stem_wgrad(act(64), torch.zeros(N, H, W, 16, dtype=BF), 2 * H, 2 * W, F32),
    "stem_wgrad_bn": lambda C_: C_.stem_wgrad_bn(act(64, H // 2, W // 2), pos(64), act(64), ws(64),
                                                 torch.zeros(N, H, W, 16, dtype=BF), 2 * H, 2 * W, F32),
}


def _bound_tensor_ops():
    """Names bound in bind_nn whose pybind signature takes a tensor."""
    C_ = _ext.require()
    src = open(os.path.join(ROOT, "csrc", "nn_bindings.cpp")).read()
    names = re.findall(r'm\.def\("([a-z0-9_]+)"', src[src.index("void bind_nn("):])
    assert names, "no m.def found in bind_nn (pattern broken?)"
    return sorted(n for n in names if "Tensor" in (getattr(C_, n).__doc__ or "").split("->")[0])


def test_every_tensor_op_of_bind_nn_is_covered():
    assert _bound_tensor_ops() == sorted(CALLS)


@pytest.mark.parametrize("op", sorted(CALLS))
def test_host_tensors_are_refused(op):
    with pytest.raises(RuntimeError):
        CALLS[op](_ext.require())


# ---- maxpool_bwd: window, image size and dy's size are checked from the arguments alone, before the device check,
# so host tensors show them. (dy [N, C, oh, ow] dtype, H, W, k, s, p) -> the message
MAXPOOL_BWD_REFUSED = [
    ((2, 2, BF), 4, 4, 3, 0, 1, "unsupported window"),        # s = 0 would divide by zero on the device
    ((2, 2, BF), 4, 4, 16, 2, 1, "unsupported window"),       # k > 15 leaves the position byte
    ((2, 2, BF), 4, 4, 0, 2, 0, "unsupported window"),
    ((2, 2, BF), 4, 4, 3, 2, 2, "unsupported window"),        # 2p > k
    ((2, 2, BF), 4, 4, 3, 2, -1, "unsupported window"),
    ((2, 2, BF), 0, 4, 3, 2, 1, "H and W must be positive"),
    ((2, 2, BF), 4, -4, 3, 2, 1, "H and W must be positive"),
    ((2, 2, BF), 5, 4, 3, 2, 1, "is not the pooled size"),    # 5 rows pool to 3, floor and ceil
    ((2, 2, BF), 4, 7, 3, 2, 1, "is not the pooled size"),    # 7 columns pool to 4
    ((2, 4, BF), 4, 4, 3, 2, 1, "is not the pooled size"),    # 4 columns pool to 2 (floor) or 3 (ceil)
    ((64, 64, BF), 1 << 16, 1 << 16, 1, 1024, 0, "too large for 32-bit indexing"),
    ((2, 2, torch.float16), 4, 4, 3, 2, 1, "dy must be bf16 or fp32"),
    ((2, 2, torch.float64), 4, 4, 3, 2, 1, "dy must be bf16 or fp32"),
]


@pytest.mark.parametrize("dy,h,w,k,s,p,msg", MAXPOOL_BWD_REFUSED)
def test_maxpool_bwd_refuses_bad_geometry(dy, h, w, k, s, p, msg):
    oh, ow, dt = dy
    with pytest.raises(RuntimeError, match=f"maxpool_bwd: .*{msg}"):
        _ext.require().maxpool_bwd(act(h=oh, w=ow, dtype=dt), pos(h=oh, w=ow), h, w, k, s, p)


def test_maxpool_bwd_accepts_floor_and_ceil_sizes():
    """[2, 2] is the floor-mode and [3, 3] the ceil-mode pooled size of a 6 x 6 image under 3x3/s2/p0: both pass the
    geometry checks and reach the device check."""
    for o in (2, 3):
        with pytest.raises(RuntimeError, match="dy must be a GPU tensor"):
            _ext.require().maxpool_bwd(act(h=o, w=o), pos(h=o, w=o), 6, 6, 3, 2, 0)


def test_pool_fast_index_is_fdivs_domain():
    """The multiply-shift index decode of the pool kernels only with work < 2^24 AND every divisor < 2^16."""
    f = _ext.require().pool_fast_index
    assert f((1 << 24) - 1, 3, 2365, 2364) and not f(1 << 24, 3, 2365, 2364)
    assert f(100, 65535, 1, 1) and not f(100, 65536, 1, 1) and not f(100, 1, 65536, 1) and not f(100, 1, 1, 65536)
    assert not f(2 * 1048577, 1, 1048577, 2)  # a [1, 8, 2, 1048577] image
