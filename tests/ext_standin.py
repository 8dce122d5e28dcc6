"""A torch stand-in for the extension calls of the 1x1 conv -> BN(+identity)+ReLU hand-off path, so the autograd
Functions and link classes of ops/conv.py and ops/bn_act.py run on the CPU (tests/test_handoff_links.py).

It answers the calls the way the bindings do as far as the Python layer can tell: same argument order, same
tuple shapes, bf16 results, the ReLU mask as packed bits in channels_last element order, the residual addend of
the data gradient masked by such bits. The one-pass gradient kernel reports "not served" (an empty list), so a
parked BN gradient is materialised through ``bn_act_bwd``. The arithmetic is fp32 torch; only mask modes 0 (no
ReLU) and 2 (bit mask) are modelled."""
import torch
import torch.nn.functional as F


def pack_bits(b: torch.Tensor) -> torch.Tensor:
    """0/1 values in element order -> bytes, element 8 i + j in bit j of byte i."""
    b = F.pad(b.reshape(-1).to(torch.uint8), (0, -b.numel() % 8)).view(-1, 8).to(torch.int32)
    return (b << torch.arange(8, dtype=torch.int32)).sum(1).to(torch.uint8)


def unpack_bits(mask: torch.Tensor, shape) -> torch.Tensor:
    bits = torch.stack([(mask >> j) & 1 for j in range(8)], 1).reshape(-1)
    return bits[: torch.Size(shape).numel()].view(shape).float()


def _nhwc(t):  # [N, C, H, W] channels_last -> [N, H, W, C] contiguous view
    return t.permute(0, 2, 3, 1)


class StandIn:
    def __init__(self):
        self.calls = []

    def gemm_nt(self, A, W, stats, addend=None, kmajor=False, tile=0, amask=None, dsub=None, h=0, w=0):
        self.calls.append("gemm_nt")
        assert dsub is None
        out = A.float() @ (W.float() if kmajor else W.float().t())
        if addend is not None:
            out = out + (addend.float() if amask is None else addend.float() * unpack_bits(amask, addend.shape))
        return out.to(A.dtype), None

    def gemm_tn(self, A, B, odt, scale):
        self.calls.append("gemm_tn")
        return (A.float().t() @ B.float() * scale).to(odt)

    def conv1x1_dual_bn_ok(self, M, ci, co):
        return True

    def conv1x1_dual_blocks(self, M, ci, co):
        return 0

    def conv1x1_dual(self, *a):
        self.calls.append("conv1x1_dual")
        return []

    def bn_act_fwd(self, x, res, w, b, rm, rv, training, mom, eps, relu, stats, _n, _z, defer):
        self.calls.append("bn_act_fwd")
        assert not defer
        y = F.batch_norm(x.float(), rm, rv, w, b, training, mom, eps)
        if res is not None:
            y = y + res.float()
        mask = pack_bits(_nhwc(y > 0)) if relu and res is not None else None
        y = y.clamp_min(0) if relu else y
        ws = torch.tensor([eps, mom])
        return y.to(x.dtype).contiguous(memory_format=torch.channels_last), ws, mask

    def bn_act_bwd(self, dy, _n, mask, x, ws, w, mode, want_res, ext, want_dx=True):
        self.calls.append("bn_act_bwd")
        assert mode in (0, 2) and ext is None and (mask is not None) == (mode == 2)
        g = dy.float()
        if mode == 2:
            g = g * unpack_bits(mask, _nhwc(x).shape).permute(0, 3, 1, 2)
        xf, dims, v = x.float(), (0, 2, 3), (1, -1, 1, 1)
        rstd = (xf.var(dims, unbiased=False) + float(ws[0])).rsqrt()
        xhat = (xf - xf.mean(dims).view(v)) * rstd.view(v)
        dg, db = (g * xhat).sum(dims), g.sum(dims)
        m = xf.numel() // xf.shape[1]
        dx = (w * rstd).view(v) * (g - db.view(v) / m - xhat * dg.view(v) / m)
        cl = torch.channels_last
        return (dx.to(x.dtype).contiguous(memory_format=cl) if want_dx else None,
                g.to(x.dtype).contiguous(memory_format=cl) if want_res else None, dg, db)
