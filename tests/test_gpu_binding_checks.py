"""Argument checks of csrc/nn_bindings.cpp on the GPU: one case per shared check helper per op that uses it, each
a well-formed call with one argument malformed, which must be refused with a RuntimeError that names the op and
the argument; and the well-formed call of each op family itself, which must not be refused.

Apart from the host-tensor cases every malformed argument is mis-typed, mis-strided or too large, never too small:
its storage covers whatever the kernel could touch, so a missing check would show as a wrong result and a failed
assertion here, not as a stray access. The host-tensor cases rely on the check preceding every launch of the op
(check_ws / f32_vec / check_bitmask run while the launcher's arguments are formed)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N, C, H, W = 2, 16, 4, 4
M = N * H * W
BF, F32 = torch.bfloat16, torch.float32


class Args:
    """Well-formed arguments of every op under test, built once per module on the device."""

    def __init__(self, dev):
        from distributed_learning_amd.ops import _ext

        self.C = _ext.require()
        g = torch.Generator().manual_seed(3)

        def act(c=C, h=H, w=W):
            return torch.randn(N, c, h, w, generator=g).to(dev, BF).contiguous(memory_format=torch.channels_last)

        def mat(r, c):
            return torch.randn(r, c, generator=g).to(dev, BF)

        def vec():
            return (torch.rand(C, generator=g) + 0.5).to(dev)

        x, xd, dy = act(), act(), act()
        gamma, beta, rm, rv = vec(), vec(), torch.zeros(C, device=dev), torch.ones(C, device=dev)
        y, ws, mask = self.C.bn_act_fwd(x, xd, gamma, beta, rm, rv, True, 0.1, 1e-5, True)
        yd, wsa, wsd, maskd = self.C.bn_dual_fwd(x, xd, gamma, beta, rm, rv, gamma, beta, rm.clone(), rv.clone(), 0.1,
                                                 0.1, 1e-5, 1e-5, True, None, None)
        yp, wsp, pos = self.C.bn_relu_maxpool_fwd(x, gamma, beta, rm, rv, 0.1, 1e-5, 3, 2, 1)
        dyp = act(h=H // 2, w=W // 2)
        mp, mpos = self.C.maxpool_fwd(x, 3, 2, 1)
        stats = torch.zeros(1, C, 2, device=dev)
        A, B, Bk = mat(M, C), mat(M, C), mat(C, M)  # gemm_nt: [32, 16] x [32, 16]^T; k-major B [16, 32]
        addend, xbn = mat(M, M), mat(M, M)
        bits_mm = torch.zeros(M * M // 8, dtype=torch.uint8, device=dev)
        ws_m = torch.zeros(7 * M, device=dev)
        ws_m[M:2 * M] = 1.0
        w3 = (torch.randn(C, C, 3, 3, generator=g) * 0.1).to(dev, BF).contiguous(memory_format=torch.channels_last)
        # op -> [function, positional arguments]
        self.calls = {
            "bn_act_fwd": [self.C.bn_act_fwd, [x, xd, gamma, beta, rm, rv, True, 0.1, 1e-5, True, stats]],
            "bn_act_bwd": [self.C.bn_act_bwd, [dy, None, mask, x, ws.clone(), gamma, 2, False, None]],
            "bn_dual_fwd": [self.C.bn_dual_fwd, [x, xd, gamma, beta, rm, rv, gamma, beta, rm.clone(), rv.clone(), 0.1,
                                                 0.1, 1e-5, 1e-5, True, stats, stats]],
            "bn_dual_bwd": [self.C.bn_dual_bwd, [dy, maskd, x, wsa.clone(), gamma, xd, wsd.clone(), gamma]],
            "bn_apply_deferred": [self.C.bn_apply_deferred, [x, xd, wsa, wsd, torch.empty_like(x),
                                                             torch.empty_like(maskd)]],
            "bn_relu_maxpool_fwd": [self.C.bn_relu_maxpool_fwd, [x, gamma, beta, rm, rv, 0.1, 1e-5, 3, 2, 1, stats]],
            "bn_relu_maxpool_bwd": [self.C.bn_relu_maxpool_bwd, [dyp, pos, x, wsp.clone(), gamma, 3, 2, 1]],
            "maxpool_bwd": [self.C.maxpool_bwd, [dyp, mpos, H, W, 3, 2, 1]],
            "bn_group_fwd": [self.C.bn_group_fwd, [[x], [gamma], [beta], [rm], [rv], [0.1], [1e-5], [stats]]],
            "bn_group_bwd": [self.C.bn_group_bwd, [[dy], [x], [gamma], [ws.clone()], []]],
            "bn_concat_fwd": [self.C.bn_concat_fwd, [[x], [gamma], [beta], [rm], [rv], [0.1], [1e-5], [stats],
                                                     torch.empty_like(x)]],
            "bn_concat_bwd": [self.C.bn_concat_bwd, [dy, [x], [gamma], [ws.clone()]]],
            "gemm_nt": [self.C.gemm_nt, [A, B, False, addend, False, 0, bits_mm]],
            "gemm_nt_bn": [self.C.gemm_nt_bn, [A, Bk, None, True, xbn, ws_m, bits_mm, 2]],
            "gemm_tn": [self.C.gemm_tn, [A, B, F32]],
            "conv3x3_dgrad_bn": [self.C.conv3x3_dgrad_bn, [dy, w3, None, x, ws.clone(), mask, 2]],
            "conv3x3_wgrad": [self.C.conv3x3_wgrad, [dy, x, 1, F32]],
        }
        # refused before any shape gate, so never launched: the same small shapes serve
        m64 = torch.zeros(M, C, dtype=BF, device=dev)
        bits = torch.zeros(M * C // 8, dtype=torch.uint8, device=dev)
        ws_c = torch.zeros(7 * C, device=dev)
        xs = torch.zeros(N, H, W, 16, dtype=BF, device=dev)
        self.gated = {
            "gemm_nt_apply": [self.C.gemm_nt_apply, [m64, m64, ws_c, ws_c, mat(M, C), True, m64.clone(), bits]],
            "gemm_nt_stream_apply": [self.C.gemm_nt_stream_apply, [m64, ws_c, mat(M, C), m64.clone()]],
            "conv1x1_dual": [self.C.conv1x1_dual, [mat(M, C), mat(M, C), mat(C, C), F32]],
            "stem_wgrad": [self.C.stem_wgrad, [act(64), xs, 2 * H, 2 * W, F32]],
            "stem_wgrad_bn": [self.C.stem_wgrad_bn, [dyp, pos, x, wsp.clone(), xs, 2 * H, 2 * W, F32]],
        }


@pytest.fixture(scope="module")
def args(cuda):
    return Args(cuda)


# ---- the malformed forms: each takes the well-formed tensor ----
def longer(t):  # ws of 7C + 7 elements, weight of 2C elements
    return torch.cat([t, t[:7] if t.numel() > 7 * 8 else t])


def fp64(t):
    return t.double()


def strided(t):  # a stride-2 view of a vector twice as long
    return torch.cat([t, t])[::2]


def int16(t):  # at least as many bytes
    return torch.zeros(t.numel(), dtype=torch.int16, device=t.device)


def host(t):
    return t.cpu()


def three(t):  # partials [rows, C, 3]
    return torch.zeros(t.shape[0], t.shape[1], 3, device=t.device)


def plain_strides(t):  # pos with contiguous instead of channels_last strides
    return t.contiguous(memory_format=torch.contiguous_format)


WS = [longer, fp64, host]
WEIGHT = [longer, strided, host]
MASK = [int16, host]

# (op, index of the argument, its name in the message, malformed forms); a list argument is malformed in element 0
CASES = [
    ("bn_act_fwd", 2, "weight", WEIGHT), ("bn_act_fwd", 5, "running_var", WEIGHT), ("bn_act_fwd", 10, "stats", [three]),
    ("bn_act_bwd", 4, "ws", WS), ("bn_act_bwd", 5, "weight", WEIGHT), ("bn_act_bwd", 2, "mask", MASK),
    ("bn_dual_fwd", 2, "weight", WEIGHT), ("bn_dual_fwd", 6, "weight", WEIGHT), ("bn_dual_fwd", 16, "stats", [three]),
    ("bn_dual_bwd", 3, "ws", WS), ("bn_dual_bwd", 6, "wsd", WS), ("bn_dual_bwd", 4, "weight", WEIGHT),
    ("bn_dual_bwd", 7, "weight_d", WEIGHT), ("bn_dual_bwd", 1, "mask", MASK),
    ("bn_apply_deferred", 2, "ws", WS), ("bn_apply_deferred", 3, "wsd", WS), ("bn_apply_deferred", 5, "mask", MASK),
    ("bn_relu_maxpool_fwd", 1, "weight", WEIGHT), ("bn_relu_maxpool_fwd", 10, "stats", [three]),
    ("bn_relu_maxpool_bwd", 3, "ws", WS), ("bn_relu_maxpool_bwd", 4, "weight", WEIGHT),
    ("bn_relu_maxpool_bwd", 1, "pos", [plain_strides]),
    ("maxpool_bwd", 1, "pos", [plain_strides]),
    ("bn_group_fwd", 1, "weight", WEIGHT), ("bn_group_fwd", 7, "stats", [three]),
    ("bn_group_bwd", 3, "ws", WS), ("bn_group_bwd", 2, "weight", WEIGHT),
    ("bn_concat_fwd", 4, "running_var", WEIGHT), ("bn_concat_fwd", 7, "stats", [three]),
    ("bn_concat_bwd", 3, "ws", WS), ("bn_concat_bwd", 2, "weight", WEIGHT),
    ("gemm_nt", 6, "addend_mask", MASK),
    ("gemm_nt_bn", 5, "ws", WS), ("gemm_nt_bn", 6, "mask", MASK),
    ("conv3x3_dgrad_bn", 4, "ws", WS), ("conv3x3_dgrad_bn", 5, "mask", MASK),
    ("gemm_nt_apply", 2, "ws", WS), ("gemm_nt_apply", 3, "wsd", WS), ("gemm_nt_apply", 7, "mask", MASK),
    ("gemm_nt_stream_apply", 1, "ws", WS),
    ("stem_wgrad_bn", 3, "ws", WS), ("stem_wgrad_bn", 1, "pos", [plain_strides]),
]
FP16 = [("gemm_tn", 2), ("conv3x3_wgrad", 3), ("conv1x1_dual", 3), ("stem_wgrad", 4), ("stem_wgrad_bn", 7)]


def _flat():
    for op, idx, name, forms in CASES:
        for form in forms:
            yield pytest.param(op, idx, name, form, id=f"{op}-{name}{idx}-{form.__name__}")


def _call(args, op):
    fn, a = (args.calls.get(op) or args.gated[op])
    return fn, [v.clone() if torch.is_tensor(v) else list(v) if isinstance(v, list) else v for v in a]


@pytest.mark.parametrize("op,idx,name,form", list(_flat()))
def test_malformed_argument_is_refused(args, op, idx, name, form):
    fn, a = _call(args, op)
    if isinstance(a[idx], list):
        a[idx] = [form(a[idx][0])] + a[idx][1:]
    else:
        a[idx] = form(a[idx])
    op_in_message = {"bn_group_fwd": "grouped BN", "bn_concat_fwd": "grouped BN", "bn_group_bwd": "grouped BN backward",
                     "bn_concat_bwd": "grouped BN backward"}.get(op, op)
    with pytest.raises(RuntimeError, match=rf"{op_in_message}.*: {name} must"):
        fn(*a)
    torch.cuda.synchronize()


@pytest.mark.parametrize("op,idx", FP16)
def test_fp16_output_is_refused(args, op, idx):
    fn, a = _call(args, op)
    a[idx] = torch.float16
    with pytest.raises(RuntimeError, match=rf"{op}: out_dtype must be fp32 or bf16"):
        fn(*a)


def test_epilogue_partials_of_the_backwards_are_checked(args):
    """ext_part / exts are absent from the well-formed calls (a reduction pass runs instead)."""
    fn, a = _call(args, "bn_group_bwd")
    a[4] = [torch.zeros(1, C, 3, device=a[0][0].device)]
    with pytest.raises(RuntimeError, match="bn_group_bwd: exts must"):
        fn(*a)
    fn, a = _call(args, "bn_act_bwd")
    a[8] = torch.zeros(1, C, 3, device=a[0].device)
    with pytest.raises(RuntimeError, match="bn_act_bwd: ext_part must"):
        fn(*a)


def test_well_formed_calls_are_accepted(args):
    """The same arguments, nothing malformed: the checks refuse no op family's normal call."""
    for op in args.calls:
        fn, a = _call(args, op)
        fn(*a)
    torch.cuda.synchronize()


# ---- maxpool_bwd's geometry (the table of test_binding_checks.py, here with well-formed device tensors: refused
# before any launch) ----
MAXPOOL_BWD_REFUSED = [
    ((2, 2, BF), 4, 4, 3, 0, 1, "unsupported window"),
    ((2, 2, BF), 4, 4, 16, 2, 1, "unsupported window"),
    ((2, 2, BF), 4, 4, 3, 2, 2, "unsupported window"),
    ((2, 2, BF), 0, 4, 3, 2, 1, "H and W must be positive"),
    ((2, 2, BF), 5, 4, 3, 2, 1, "is not the pooled size"),
    ((2, 4, BF), 4, 4, 3, 2, 1, "is not the pooled size"),
    ((64, 64, BF), 1 << 16, 1 << 16, 1, 1024, 0, "too large for 32-bit indexing"),
    ((2, 2, torch.float16), 4, 4, 3, 2, 1, "dy must be bf16 or fp32"),
]


@pytest.mark.parametrize("dy,h,w,k,s,p,msg", MAXPOOL_BWD_REFUSED)
def test_maxpool_bwd_refuses_bad_geometry(args, cuda, dy, h, w, k, s, p, msg):
    oh, ow, dt = dy
    d = torch.zeros(N, C, oh, ow, dtype=dt, device=cuda).contiguous(memory_format=torch.channels_last)
    ps = torch.zeros(N, C, oh, ow, dtype=torch.uint8, device=cuda).contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match=f"maxpool_bwd: .*{msg}"):
        args.C.maxpool_bwd(d, ps, h, w, k, s, p)
    torch.cuda.synchronize()


def test_fused_bn_pool_refuses_divisors_outside_the_fast_division(args, cuda):
    """The fused BN+ReLU+max-pool kernels decode indices by multiply-shift only: a 65536-wide image is refused."""
    x = torch.zeros(1, 8, 1, 65536, dtype=BF, device=cuda).contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match="bn_relu_maxpool: H, W and C / 8 must be below 65536"):
        args.C.bn_relu_maxpool_fwd(x, None, None, None, None, 0.1, 1e-5, 3, 2, 1)
    dyp = torch.zeros(1, 8, 1, 32768, dtype=BF, device=cuda).contiguous(memory_format=torch.channels_last)
    ps = torch.zeros(1, 8, 1, 32768, dtype=torch.uint8, device=cuda).contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match="bn_relu_maxpool_bwd: .*below 65536"):
        args.C.bn_relu_maxpool_bwd(dyp, ps, x, torch.zeros(56, device=cuda), None, 3, 2, 1)
    torch.cuda.synchronize()


# ---- the stride-2 second addend: its epilogue decodes (n, h, w) from the output row by multiply-shift (mm::fdiv) ----
# (op, n, H, W): a 65536-row image, and 2^24 rows; every argument well-formed apart from the size
ADDEND2_REFUSED = [("gemm_nt", 1, 65536, 2), ("gemm_nt_bn", 1, 65536, 2), ("gemm_nt", 1, 2, 65536), ("gemm_nt", 1 << 22, 2, 2)]


@pytest.mark.parametrize("op,n,h,w", ADDEND2_REFUSED)
def test_addend2_refuses_rows_outside_the_fast_division(args, cuda, op, n, h, w):
    m, c = n * h * w, 8
    A, Bk = torch.zeros(m, c, dtype=BF, device=cuda), torch.zeros(c, c, dtype=BF, device=cuda)
    a2 = torch.zeros(n, h // 2, w // 2, c, dtype=BF, device=cuda).permute(0, 3, 1, 2)  # channels_last [n, C, H/2, W/2]
    with pytest.raises(RuntimeError, match=rf"{op}: addend2 needs .*24-bit index math"):
        if op == "gemm_nt":
            args.C.gemm_nt(A, Bk, False, None, True, 0, None, a2, h, w)
        else:
            args.C.gemm_nt_bn(A, Bk, None, True, torch.zeros(m, c, dtype=BF, device=cuda), torch.zeros(7 * c, device=cuda),
                              None, 1, None, a2, h, w)
    torch.cuda.synchronize()


# ---- the divisor bound of the multiply-shift decodes (mm::fdiv: dividend < 2^24 AND divisor < 2^16) in the conv, stem
# and fp32-conv bindings. These checks follow the device check, so tests/test_binding_checks.py cannot see them; the
# operands are uninitialised and nothing is launched. The same refusals at 2^24 pixels and 2^31 bytes:
# tests/test_gpu_index_edges.py ----
def _cl_empty(dev, n, c, h, w, dtype=BF):
    return torch.empty(n, h, w, c, dtype=dtype, device=dev).permute(0, 3, 1, 2)


# [1, 8, 254, 66011] is the geometry whose last pixel decodes to a row outside the image (tests/test_index_domain.py)
DIVISOR_REFUSED = [(1, 8, 254, 66011), (1, 8, 66011, 254), (1, 8, 1, 65536), (1, 8, 65536, 1)]


@pytest.mark.parametrize("shape", DIVISOR_REFUSED)
def test_conv3x3_refuses_divisors_outside_the_fast_division(args, cuda, shape):
    x = _cl_empty(cuda, *shape)
    w = torch.empty(8, 8, 3, 3, dtype=BF, device=cuda).contiguous(memory_format=torch.channels_last)
    ws = torch.zeros(7 * 8, device=cuda)
    for call in (lambda: args.C.conv3x3_fwd(x, w, 1, True), lambda: args.C.conv3x3_dgrad(x, w),
                 lambda: args.C.conv3x3_dgrad_bn(x, w, None, x, ws, None, 1)):
        with pytest.raises(RuntimeError, match="conv3x3: H, W, Cin and Cout must be below 65536"):
            call()
    with pytest.raises(RuntimeError, match="conv3x3_wgrad: H and W must be below 65536"):
        args.C.conv3x3_wgrad(x, x, 1, F32)
    torch.cuda.synchronize()


def test_conv3x3_accepts_the_largest_divisor(args, cuda):
    """[1, 8, 1, 65535]: one step inside the bound the call runs (and test_gpu_index_edges.py checks what it computes
    at [1, 8, 255, 65535])."""
    x = torch.zeros(1, 1, 65535, 8, dtype=BF, device=cuda).permute(0, 3, 1, 2)
    w = torch.zeros(8, 8, 3, 3, dtype=BF, device=cuda).contiguous(memory_format=torch.channels_last)
    y, _ = args.C.conv3x3_fwd(x, w, 1, False)
    assert y.shape == (1, 8, 1, 65535) and not bool(y.any())


def test_channel_divisors_are_refused(args, cuda):
    """The k -> (tap, channel) decode divides by Cin (data gradient: Cout)."""
    x = _cl_empty(cuda, 1, 65536, 2, 2)
    w = torch.empty(8, 65536, 3, 3, dtype=BF, device=cuda).contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match="conv3x3: H, W, Cin and Cout must be below 65536"):
        args.C.conv3x3_fwd(x, w, 1, False)
    with pytest.raises(RuntimeError, match="conv3x3: H, W, Cin and Cout must be below 65536"):
        args.C.conv3x3_dgrad(_cl_empty(cuda, 1, 8, 2, 2), w)  # dy [1, 8, 2, 2] -> dx [1, 65536, 2, 2]
    xf = _cl_empty(cuda, 1, 65536, 2, 2, F32)
    with pytest.raises(RuntimeError, match="conv_f32_fwd: OH, OW, C and S must be below 65536"):
        args.C.conv_f32_fwd(xf, torch.empty(4, 1, 1, 65536, device=cuda), 0, 1)
    torch.cuda.synchronize()


@pytest.mark.parametrize("h,w", [(508, 132022), (2, 131072), (131071, 2)])
def test_stem_refuses_folded_sizes_outside_the_fast_division(args, cuda, h, w):
    """The stem decodes over the folded image [(H + 1) / 2, (W + 1) / 2]; 508 x 132022 folds to 254 x 66011."""
    oh, ow = (h + 1) // 2, (w + 1) // 2
    with pytest.raises(RuntimeError, match="stem_fwd: the folded BH, BW must be below 65536"):
        args.C.stem_fwd(_cl_empty(cuda, 1, 3, h, w), torch.empty(64, 256, dtype=BF, device=cuda), True)
    xs = torch.empty(1, oh, ow, 16, dtype=BF, device=cuda)
    with pytest.raises(RuntimeError, match="stem_wgrad: the folded BH, BW must be below 65536"):
        args.C.stem_wgrad(_cl_empty(cuda, 1, 64, oh, ow), xs, h, w, F32)
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", [(1, 4, 254, 66011), (1, 4, 1, 65536), (1, 4, 65536, 1)])
def test_conv_f32_refuses_divisors_outside_the_fast_division(args, cuda, shape):
    x = _cl_empty(cuda, *shape, dtype=F32)
    with pytest.raises(RuntimeError, match="conv_f32_fwd: OH, OW, C and S must be below 65536"):
        args.C.conv_f32_fwd(x, torch.empty(4, 3, 3, 4, device=cuda), 1, 1)
    with pytest.raises(RuntimeError, match="conv_f32_wgrad: OH, OW, C and S must be below 65536"):
        args.C.conv_f32_wgrad(x, x, 3, 3, 1, 1)
    torch.cuda.synchronize()


@pytest.mark.parametrize("h,w", [(131072, 4), (4, 131072)])
def test_stem_wgrad_bn_refuses_folded_sizes_outside_the_fast_division(args, cuda, h, w):
    """The fused form walks 2x2 quads of the folded image with divisors BW / 2 and BH / 2; same bound as stem_wgrad."""
    bh, bw = h // 2, w // 2
    dyp = _cl_empty(cuda, 1, 64, bh // 2, bw // 2)
    pos = torch.empty(1, bh // 2, bw // 2, 64, dtype=torch.uint8, device=cuda).permute(0, 3, 1, 2)
    xs = torch.empty(1, bh, bw, 16, dtype=BF, device=cuda)
    with pytest.raises(RuntimeError, match="stem_wgrad_bn: the folded BH, BW must be below 65536"):
        args.C.stem_wgrad_bn(dyp, pos, _cl_empty(cuda, 1, 64, bh, bw), torch.zeros(7 * 64, device=cuda), xs, h, w, F32)
    torch.cuda.synchronize()
