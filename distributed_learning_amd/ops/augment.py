"""Device-side input transform: raw uint8 HWC batches -> normalised channels-last training tensors.

One kernel (csrc/kernels/augment.hip) does per-sample crop, bilinear resample, horizontal flip, normalise,
cast and layout in a single pass, so a real-data batch reaches the model in the form
:class:`~distributed_learning_amd.data.SyntheticBatches` writes (bf16 NHWC) after one uint8 H2D copy.

Definition, shared by the kernel and the CPU implementation below. For output pixel ``(n, oy, ox, c)`` with
``geom[n] = (y0, x0, step_y, step_x)`` in source pixels, all in fp32::

    ox' = Wo-1-ox if flip[n] else ox
    sy  = (y0 - 0.5) + (oy + 0.5) * step_y          (sx likewise with ox')
    ty  = floor(sy), fy = sy - ty; taps ty and ty+1, each clamped to [-pad, Hs-1+pad];
          a clamped tap outside [0, Hs) reads 0     (x likewise)
    v   = bilinear blend of the four taps, weights (1-fy, fy) x (1-fx, fx)
    out = fmaf(v, scale_c, bias_c),  scale_c = 1 / (255 std_c),  bias_c = -mean_c / std_c

``pad = 0`` clamps at the edges (random-resized crop); ``pad = p`` with step 1 and integer offsets in
``[-p, p]`` is a crop of the image padded with ``p`` black pixels (torchvision ``RandomCrop(padding=p)``).
With step 1 and integer offsets ``fy = fx = 0``: the blend is one source byte and the result
``fmaf(byte, scale, bias)`` is bit-reproducible.

The crop boxes and flips of a batch come from :class:`AugmentParams`, a pure function of
``(seed, stream, step)`` computed on the host.

:func:`augment_mix` is the same pass with Mixup / CutMix: every sample is combined with a partner image that is
sampled with its own geometry (mixed instantiations of the same kernel); :class:`MixParams` draws its per-batch
parameters, again as a pure function of ``(seed, stream, step)``.

Both take ``index=``: ``src`` is then a resident store ``[P, Hs, Ws, 3]`` of any size (a rank's whole data shard in
HBM, :class:`~distributed_learning_amd.data.ResidentStore`) and batch image ``n`` is store row ``index[n]``, read
in place by indexed instantiations of the same kernel -- no gathered batch is ever written. The result is, bit
for bit, the un-indexed call on ``src[index]``.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import _ext
from .limits import SPAN_LIMIT, NativeLimitError

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CIFAR10_MEAN, CIFAR10_STD = (0.4914, 0.4822, 0.4465), (0.2470, 0.2435, 0.2616)

KINDS = ("rrc", "padcrop", "center")
RATIO = (3.0 / 4.0, 4.0 / 3.0)  # aspect-ratio range of the random-resized crop
ATTEMPTS = 10

_COEFF: Dict[tuple, Tuple[torch.Tensor, torch.Tensor]] = {}


def scale_bias(mean: Sequence[float], std: Sequence[float]) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(1 / (255 std), -mean / std)`` computed in float64 and rounded to fp32, on the CPU."""
    m, s = torch.tensor(mean, dtype=torch.float64), torch.tensor(std, dtype=torch.float64)
    if m.numel() != 3 or s.numel() != 3:
        raise ValueError("augment: mean and std must have 3 entries")
    return (1.0 / (255.0 * s)).to(torch.float32), (-m / s).to(torch.float32)


def _coefficients(mean, std, device) -> Tuple[torch.Tensor, torch.Tensor]:
    key = (tuple(float(v) for v in mean), tuple(float(v) for v in std), str(device))
    if key not in _COEFF:
        sc, bi = scale_bias(*key[:2])
        _COEFF[key] = (sc.to(device), bi.to(device))
    return _COEFF[key]


def _elements_ok(n: int, what: str) -> None:
    if n >= SPAN_LIMIT:
        raise NativeLimitError(f"{what}: {n} elements >= 2^31, beyond the augment kernel's 32-bit element index; "
                               f"lower the per-GPU batch")


def _check(src, geom, flip, out_hw, dtype, pad, index=None) -> int:
    """Returns the batch size: ``src``'s, or with ``index`` (``src`` is a store) the index's length."""
    if src.dtype != torch.uint8:
        raise TypeError(f"augment: src must be uint8, got {src.dtype}")
    if src.dim() != 4 or src.shape[3] != 3:
        raise ValueError(f"augment: src must be [N, Hs, Ws, 3] (HWC, 3 channels), got {tuple(src.shape)}")
    if not src.is_contiguous():
        raise ValueError("augment: src must be contiguous")
    n = src.shape[0]
    if index is not None:
        if index.dtype != torch.int32 or index.dim() != 1:
            raise ValueError(f"augment: index must be int32 [N], got {index.dtype} {tuple(index.shape)}")
        rows, n = n, index.shape[0]
        if rows < 1:
            raise ValueError("augment: an indexed store must hold at least one image")
        if index.device.type == "cpu" and n and not bool(((index >= 0) & (index < rows)).all()):
            raise ValueError(f"augment: index must be in [0, {rows})")
    if tuple(geom.shape) != (n, 4) or geom.dtype != torch.float32:
        raise ValueError(f"augment: geom must be fp32 [{n}, 4], got {geom.dtype} {tuple(geom.shape)}")
    if tuple(flip.shape) != (n,) or flip.dtype != torch.uint8:
        raise ValueError(f"augment: flip must be uint8 [{n}], got {flip.dtype} {tuple(flip.shape)}")
    if dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"augment: output dtype must be bf16 or fp32, got {dtype}")
    if len(out_hw) != 2 or min(out_hw) < 1 or min(src.shape[1:3]) < 1:
        raise ValueError(f"augment: bad sizes {tuple(src.shape)} -> {tuple(out_hw)}")
    if int(pad) < 0:
        raise ValueError(f"augment: pad must be >= 0, got {pad}")
    # an indexed store is addressed per image (64-bit base, 32-bit offsets inside): only one image is limited
    _elements_ok(src[0].numel() if index is not None else src.numel(), "augment src")
    _elements_ok(n * 3 * out_hw[0] * out_hw[1], "augment out")
    return n


def augment(src_u8: torch.Tensor, geom: torch.Tensor, flip: torch.Tensor, mean: Sequence[float],
            std: Sequence[float], out_hw: Tuple[int, int], dtype: torch.dtype, pad: int = 0,
            index: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``src_u8`` uint8 ``[N, Hs, Ws, 3]`` -> ``dtype`` ``[N, 3, Ho, Wo]`` in channels-last memory.

    ``index`` int32 ``[N]``: ``src_u8`` is a store ``[P, Hs, Ws, 3]`` and image ``n`` is its row ``index[n]``, read
    in place. A host index is range-checked and copied to the device; a device index is the caller's to keep in
    ``[0, P)``.

    ``geom`` fp32 ``[N, 4]`` and ``flip`` uint8 ``[N]`` may live on the host (:meth:`AugmentParams.params`); they
    are copied to ``src_u8``'s device. On a GPU this is the native kernel (a missing extension is an error);
    on the CPU a torch implementation of the same definition."""
    out_hw = (int(out_hw[0]), int(out_hw[1]))
    n = _check(src_u8, geom, flip, out_hw, dtype, pad, index)
    dev = src_u8.device
    geom, flip = geom.to(dev, non_blocking=True).contiguous(), flip.to(dev, non_blocking=True).contiguous()
    scale, bias = _coefficients(mean, std, dev)
    if dev.type != "cuda":
        if index is not None:
            src_u8 = src_u8[index.to(dev).long()]
        return _augment_torch(src_u8, geom, flip, scale, bias, out_hw, dtype, int(pad))
    C = _ext.require()
    out = torch.empty((n, out_hw[0], out_hw[1], 3), device=dev, dtype=dtype).permute(0, 3, 1, 2)
    if index is not None:
        C.augment_gather_(src_u8, index.to(dev, non_blocking=True).contiguous(), out, geom, flip, scale, bias, int(pad))
    else:
        C.augment_(src_u8, out, geom, flip, scale, bias, int(pad))
    return out


def _check_mix(n: int, partner, lam, box, out_hw, blend: bool) -> None:
    """Shapes and dtypes always; the values of tensors that live on the host (a device tensor is not read back)."""
    if tuple(partner.shape) != (n,) or partner.dtype != torch.int32:
        raise ValueError(f"augment_mix: partner must be int32 [{n}], got {partner.dtype} {tuple(partner.shape)}")
    if tuple(lam.shape) != (n,) or lam.dtype != torch.float32:
        raise ValueError(f"augment_mix: lam must be fp32 [{n}], got {lam.dtype} {tuple(lam.shape)}")
    if tuple(box.shape) != (n, 4) or box.dtype != torch.int32:
        raise ValueError(f"augment_mix: box must be int32 [{n}, 4], got {box.dtype} {tuple(box.shape)}")
    if n == 0:
        return
    ho, wo = out_hw
    if partner.device.type == "cpu" and not bool(((partner >= 0) & (partner < n)).all()):
        raise ValueError(f"augment_mix: partner must be in [0, {n})")
    if lam.device.type == "cpu":
        if not bool(((lam >= 0) & (lam <= 1)).all()):  # NaN fails too
            raise ValueError("augment_mix: lam must be in [0, 1]")
        if not blend and not bool((lam == 1).all()):
            raise ValueError("augment_mix: blend=False samples one image per pixel and needs lam == 1 everywhere")
    if box.device.type == "cpu":
        y0, x0, y1, x1 = box.unbind(1)
        if not bool(((0 <= y0) & (y0 <= y1) & (y1 <= ho) & (0 <= x0) & (x0 <= x1) & (x1 <= wo)).all()):
            raise ValueError(f"augment_mix: boxes must satisfy 0 <= y0 <= y1 <= {ho} and 0 <= x0 <= x1 <= {wo}")


def augment_mix(src_u8: torch.Tensor, geom: torch.Tensor, flip: torch.Tensor, partner: torch.Tensor,
                lam: torch.Tensor, box: torch.Tensor, mean: Sequence[float], std: Sequence[float],
                out_hw: Tuple[int, int], dtype: torch.dtype, pad: int = 0, blend: bool = True,
                index: Optional[torch.Tensor] = None) -> torch.Tensor:
    """:func:`augment` with Mixup / CutMix in the same pass. With ``A(j)`` the fp32 value :func:`augment` gives
    for source image ``j`` with ``geom[j]`` and ``flip[j]``, ``p = partner[n]`` and ``box[n] = (y0, x0, y1, x1)``
    on the output grid (independent of either image's flip)::

        w   = 0 if y0 <= oy < y1 and x0 <= ox < x1 else lam[n]
        out = fmaf(w, A(n)[oy, ox, c], (1 - w) * A(p)[oy, ox, c])       (fp32, then one cast)

    Mixup is an empty box with ``0 < lam < 1``, CutMix ``lam = 1`` with a box. ``partner`` int32 ``[N]``, ``lam``
    fp32 ``[N]`` and ``box`` int32 ``[N, 4]`` may live on the host (:meth:`MixParams.params`), where their values
    are range-checked; a device tensor's values are the caller's to keep in range. ``blend=False`` is the select
    form -- one sample per pixel, from ``n`` or ``p`` -- and needs ``lam == 1`` for every sample.

    ``index``: as in :func:`augment`; ``partner`` stays a position in the batch, so the partner of ``n`` is store
    row ``index[partner[n]]`` with ``geom[partner[n]]`` and ``flip[partner[n]]``."""
    out_hw = (int(out_hw[0]), int(out_hw[1]))
    n = _check(src_u8, geom, flip, out_hw, dtype, pad, index)
    _check_mix(n, partner, lam, box, out_hw, bool(blend))
    dev = src_u8.device
    geom, flip = geom.to(dev, non_blocking=True).contiguous(), flip.to(dev, non_blocking=True).contiguous()
    partner, lam, box = (t.to(dev, non_blocking=True).contiguous() for t in (partner, lam, box))
    scale, bias = _coefficients(mean, std, dev)
    if dev.type != "cuda":
        if index is not None:
            src_u8 = src_u8[index.to(dev).long()]
        return _augment_mix_torch(src_u8, geom, flip, partner, lam, box, scale, bias, out_hw, dtype, int(pad))
    C = _ext.require()
    out = torch.empty((n, out_hw[0], out_hw[1], 3), device=dev, dtype=dtype).permute(0, 3, 1, 2)
    if index is not None:
        C.augment_mix_gather_(src_u8, index.to(dev, non_blocking=True).contiguous(), out, geom, flip, partner, lam,
                              box, scale, bias, int(pad), bool(blend))
    else:
        C.augment_mix_(src_u8, out, geom, flip, partner, lam, box, scale, bias, int(pad), bool(blend))
    return out


def _taps(s: torch.Tensor, size: int, pad: int):
    """Both taps of one axis from the fp32 sample coordinates ``s`` [N, L]: (index0, index1, inside0, inside1,
    fraction); an index is only meaningful where its ``inside`` is set."""
    t = torch.floor(s)
    f = s - t
    t = t.clamp(-2.0 ** 30, 2.0 ** 30).to(torch.int64)
    out = []
    for tap in (t, t + 1):
        tap = tap.clamp(-pad, size - 1 + pad)
        inside = (tap >= 0) & (tap < size)
        out.append((tap.clamp(0, size - 1), inside))
    (i0, m0), (i1, m1) = out
    return i0, i1, m0, m1, f


def _augment_torch(src, geom, flip, scale, bias, out_hw, dtype, pad) -> torch.Tensor:
    return _augment_values(src, geom, flip, scale, bias, out_hw, pad).to(dtype).permute(0, 3, 1, 2)


def _augment_mix_torch(src, geom, flip, partner, lam, box, scale, bias, out_hw, dtype, pad) -> torch.Tensor:
    """The mixed definition on the CPU: both images sampled, then ``fmaf(w, a, (1 - w) * b)`` with the fp32
    product ``(1 - w) * b`` and the exact product ``w * a`` summed in float64."""
    ho, wo = out_hw
    p = partner.long()
    a = _augment_values(src, geom, flip, scale, bias, out_hw, pad)
    b = _augment_values(src[p], geom[p], flip[p], scale, bias, out_hw, pad)
    oy = torch.arange(ho, device=src.device)[None, :, None]
    ox = torch.arange(wo, device=src.device)[None, None, :]
    y0, x0, y1, x1 = (box[:, i].long()[:, None, None] for i in range(4))
    inbox = (oy >= y0) & (oy < y1) & (ox >= x0) & (ox < x1)
    w = torch.where(inbox, torch.zeros((), dtype=torch.float32), lam[:, None, None])[..., None]  # [N, Ho, Wo, 1]
    rest = (1.0 - w) * b
    out = (w.double() * a.double() + rest.double()).to(torch.float32).to(dtype)
    return out.permute(0, 3, 1, 2)


def _augment_values(src, geom, flip, scale, bias, out_hw, pad) -> torch.Tensor:
    """``A(n)``: the fp32 values ``[N, Ho, Wo, 3]`` of the plain definition."""
    n, hs, ws, _ = src.shape
    ho, wo = out_hw
    f32 = torch.float32
    oy = torch.arange(ho, dtype=f32, device=src.device)[None, :]
    ox = torch.arange(wo, dtype=f32, device=src.device)[None, :]
    ox = torch.where(flip[:, None] != 0, (wo - 1) - ox, ox)
    sy = (geom[:, 0:1] - 0.5) + (oy + 0.5) * geom[:, 2:3]
    sx = (geom[:, 1:2] - 0.5) + (ox + 0.5) * geom[:, 3:4]
    y0, y1, my0, my1, fy = _taps(sy, hs, pad)
    x0, x1, mx0, mx1, fx = _taps(sx, ws, pad)
    img = torch.arange(n, device=src.device)[:, None, None]
    fy, fx = fy[:, :, None, None], fx[:, None, :, None]

    def tap(yi, xi, my, mx):
        v = src[img, yi[:, :, None], xi[:, None, :]].to(f32)  # [N, Ho, Wo, 3]
        return v * (my[:, :, None] & mx[:, None, :])[..., None].to(f32)

    blend = (((1 - fy) * (1 - fx)) * tap(y0, x0, my0, mx0) + ((1 - fy) * fx) * tap(y0, x1, my0, mx1)) \
        + ((fy * (1 - fx)) * tap(y1, x0, my1, mx0) + (fy * fx) * tap(y1, x1, my1, mx1))
    # fmaf: the fp32 x fp32 product is exact in float64; with integer geometry so is the sum (one rounding)
    return (blend.double() * scale.double() + bias.double()).to(f32)


def boxes_to_geom(y0, x0, h, w, out_hw: Tuple[int, int]) -> torch.Tensor:
    """Crop boxes (top ``y0``, left ``x0``, height ``h``, width ``w``, in source pixels) -> fp32 ``[N, 4]`` rows
    ``(y0, x0, step_y, step_x)`` with ``step = size / output size`` in float64, rounded to fp32."""
    f64 = torch.float64
    y0, x0, h, w = (torch.as_tensor(v).to(f64).reshape(-1) for v in (y0, x0, h, w))
    return torch.stack([y0, x0, h / float(out_hw[0]), w / float(out_hw[1])], dim=1).to(torch.float32)


class AugmentParams:
    """Per-batch crop boxes and flips: ``params(step, n)`` is a pure function of ``(seed, stream, step)``.

    Every call seeds a private ``torch.Generator`` (as :class:`~distributed_learning_amd.data.EpochSampler`
    does per epoch) and never touches the global RNG, so a resumed run at batch ``k`` draws batch ``k``'s
    parameters. ``stream`` is the data partition index. Vectorised over the batch, on the host.

    kinds:

    * ``rrc`` -- torchvision ``RandomResizedCrop`` semantics: up to 10 attempts with area
      ``U(scale_min, 1) * Hs * Ws`` and log aspect ratio ``U(log 3/4, log 4/3)``,
      ``w = round(sqrt(area * r))``, ``h = round(sqrt(area / r))``, the first attempt with ``0 < w <= Ws`` and
      ``0 < h <= Hs`` taken at a position uniform over the valid integer offsets; without one, the
      ratio-clamped centre crop. Flip with p = 0.5.
    * ``padcrop`` -- the ``out_hw`` box at the centred position plus integer offsets uniform in
      ``[-pad, pad]``, step 1 (use with ``augment(..., pad=pad)``: the border reads black). Flip with p = 0.5.
    * ``center`` -- the fixed centred ``out_hw`` box, no flip: the evaluation transform.
    """

    def __init__(self, kind: str, src_hw: Tuple[int, int], out_hw: Tuple[int, int], seed: int = 1234,
                 stream: int = 0, scale_min: float = 0.08, pad: int = 0):
        if kind not in KINDS:
            raise ValueError(f"unknown augmentation kind {kind!r}; choose from {KINDS}")
        if not 0.0 < scale_min <= 1.0:
            raise ValueError(f"scale_min must be in (0, 1], got {scale_min}")
        if pad < 0:
            raise ValueError(f"pad must be >= 0, got {pad}")
        self.kind = kind
        self.src_hw = (int(src_hw[0]), int(src_hw[1]))
        self.out_hw = (int(out_hw[0]), int(out_hw[1]))
        self.seed, self.stream = int(seed), int(stream)
        self.scale_min, self.pad = float(scale_min), int(pad)

    def _generator(self, step: int) -> torch.Generator:
        s = ((self.seed * 1_000_003 + self.stream) * 2_147_483_659 + int(step)) % (1 << 63)
        return torch.Generator().manual_seed(s)

    def boxes(self, step: int, n: int):
        """Integer ``(y0, x0, h, w)`` int64 tensors and the uint8 flips of batch ``step``."""
        (hs, ws), (ho, wo) = self.src_hw, self.out_hw
        g = self._generator(step)
        cy, cx = (hs - ho) // 2, (ws - wo) // 2
        full = lambda v: torch.full((n,), v, dtype=torch.int64)  # noqa: E731
        if self.kind == "center":
            return full(cy), full(cx), full(ho), full(wo), torch.zeros(n, dtype=torch.uint8)
        if self.kind == "padcrop":
            off = torch.randint(-self.pad, self.pad + 1, (n, 2), generator=g)
            flip = (torch.rand(n, generator=g, dtype=torch.float64) < 0.5).to(torch.uint8)
            return cy + off[:, 0], cx + off[:, 1], full(ho), full(wo), flip
        f64 = torch.float64
        area = (self.scale_min + (1.0 - self.scale_min) * torch.rand(n, ATTEMPTS, generator=g, dtype=f64)) * (hs * ws)
        lo, hi = math.log(RATIO[0]), math.log(RATIO[1])
        ratio = torch.exp(lo + (hi - lo) * torch.rand(n, ATTEMPTS, generator=g, dtype=f64))
        upos = torch.rand(n, 2, generator=g, dtype=f64)
        flip = (torch.rand(n, generator=g, dtype=f64) < 0.5).to(torch.uint8)
        w = torch.round(torch.sqrt(area * ratio)).to(torch.int64)
        h = torch.round(torch.sqrt(area / ratio)).to(torch.int64)
        ok = (w > 0) & (w <= ws) & (h > 0) & (h <= hs)
        first = ok.to(torch.int64).argmax(dim=1, keepdim=True)  # first accepted attempt (0 when none is)
        w, h, found = w.gather(1, first)[:, 0], h.gather(1, first)[:, 0], ok.any(dim=1)
        y0 = torch.minimum((upos[:, 0] * (hs - h + 1).to(f64)).floor().to(torch.int64), hs - h)
        x0 = torch.minimum((upos[:, 1] * (ws - w + 1).to(f64)).floor().to(torch.int64), ws - w)
        # no attempt fits: the whole image, cut centrally to the nearest allowed aspect ratio
        fh, fw = hs, ws
        if ws / hs < RATIO[0]:
            fh = min(hs, int(round(ws / RATIO[0])))
        elif ws / hs > RATIO[1]:
            fw = min(ws, int(round(hs * RATIO[1])))
        h, w = torch.where(found, h, full(fh)), torch.where(found, w, full(fw))
        y0, x0 = torch.where(found, y0, full((hs - fh) // 2)), torch.where(found, x0, full((ws - fw) // 2))
        return y0, x0, h, w, flip

    def params(self, step: int, n: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(geom fp32 [n, 4], flip uint8 [n])`` of batch ``step``, on the host."""
        y0, x0, h, w, flip = self.boxes(step, n)
        return boxes_to_geom(y0, x0, h, w, self.out_hw), flip


class MixParams:
    """Per-batch Mixup / CutMix parameters: ``params(step, n)`` is a pure function of ``(seed, stream, step)``.

    Like :class:`AugmentParams` every call seeds a private ``torch.Generator`` and never touches a global RNG; the
    seed is mixed differently, so the crops and flips of a step are the same with and without mixing. Per batch:
    one mode (CutMix with probability ``switch_prob`` when both alphas are > 0, else the one that is set), one
    ``lam0 ~ Beta(alpha, alpha)`` of that mode (the ratio of two seeded Gamma draws) and ``partner = randperm(n)``.

    * Mixup: ``lam = target_lam = lam0``, empty boxes, ``blend = True``.
    * CutMix: a box of ``int(Ho r) x int(Wo r)``, ``r = sqrt(1 - lam0)``, around a centre uniform over the output
      grid, clipped to it; ``lam = 1``, ``target_lam = 1 - box area / (Ho Wo)`` (float64, rounded to fp32),
      ``blend = False``.

    The arrays are per sample, filled with the batch's values: :func:`augment_mix` and
    :func:`~distributed_learning_amd.ops.loss.cross_entropy_mix` take per-sample values.
    """

    def __init__(self, out_hw: Tuple[int, int], mixup_alpha: float = 0.0, cutmix_alpha: float = 0.0, seed: int = 1234,
                 stream: int = 0, switch_prob: float = 0.5):
        self.out_hw = (int(out_hw[0]), int(out_hw[1]))
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.switch_prob = float(switch_prob)
        if min(self.out_hw) < 1:
            raise ValueError(f"bad output size {out_hw}")
        if not (self.mixup_alpha >= 0.0 and self.cutmix_alpha >= 0.0):
            raise ValueError(f"mixup_alpha and cutmix_alpha must be >= 0, got {mixup_alpha} and {cutmix_alpha}")
        if self.mixup_alpha == 0.0 and self.cutmix_alpha == 0.0:
            raise ValueError("MixParams needs mixup_alpha > 0 or cutmix_alpha > 0")
        if not 0.0 <= self.switch_prob <= 1.0:
            raise ValueError(f"switch_prob must be in [0, 1], got {switch_prob}")
        self.seed, self.stream = int(seed), int(stream)

    def _generator(self, step: int) -> torch.Generator:
        s = (((self.seed * 998_244_353 + self.stream) * 4_294_967_311 + int(step)) ^ 0x5DEECE66D) % (1 << 63)
        return torch.Generator().manual_seed(s)

    def draw(self, step: int) -> Tuple[bool, float]:
        """``(cutmix, lam0)`` of batch ``step``: the mode and the Beta draw, before any box is cut."""
        return self._draw(self._generator(step))

    def _draw(self, g: torch.Generator) -> Tuple[bool, float]:
        u = float(torch.rand(1, generator=g, dtype=torch.float64))
        if self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0:
            cutmix = u < self.switch_prob
        else:
            cutmix = self.cutmix_alpha > 0.0
        alpha = self.cutmix_alpha if cutmix else self.mixup_alpha
        ga, gb = torch._standard_gamma(torch.full((2,), alpha, dtype=torch.float64), generator=g).tolist()
        lam0 = ga / (ga + gb) if ga + gb > 0.0 else 0.5  # both draws underflowed: the distribution's mean
        return cutmix, lam0

    def params(self, step: int, n: int):
        """``(partner int32 [n], lam fp32 [n], box int32 [n, 4], target_lam fp32 [n], blend)`` of batch ``step``,
        on the host: the first three and ``blend`` for :func:`augment_mix`, ``target_lam`` for the loss."""
        g = self._generator(step)
        cutmix, lam0 = self._draw(g)
        partner = torch.randperm(n, generator=g).to(torch.int32)
        ho, wo = self.out_hw
        if not cutmix:
            lam = torch.full((n,), lam0, dtype=torch.float64).to(torch.float32)
            return partner, lam, torch.zeros((n, 4), dtype=torch.int32), lam.clone(), True
        cy = int(torch.randint(0, ho, (1,), generator=g))
        cx = int(torch.randint(0, wo, (1,), generator=g))
        r = math.sqrt(1.0 - lam0)
        ch, cw = int(ho * r), int(wo * r)
        clip = lambda v, hi: max(0, min(v, hi))  # noqa: E731
        y0, y1 = clip(cy - ch // 2, ho), clip(cy + ch // 2, ho)
        x0, x1 = clip(cx - cw // 2, wo), clip(cx + cw // 2, wo)
        box = torch.tensor([[y0, x0, y1, x1]], dtype=torch.int32).repeat(n, 1)
        target = torch.full((n,), 1.0 - ((y1 - y0) * (x1 - x0)) / float(ho * wo), dtype=torch.float64)
        return partner, torch.ones(n, dtype=torch.float32), box, target.to(torch.float32), False
