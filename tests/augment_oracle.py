"""Float64 numpy oracle and shared cases of the augmentation tests (test_gpu_augment.py, test_augment_cpu.py).

Written from the definition in ops/augment.py's docstring, independently of both implementations: the kernel
and the torch CPU path are each compared with this, never with one another.
"""
import numpy as np
import torch

HS, WS = 19, 23  # 23 x 3 = 69-byte source rows: every row starts unaligned
INT_HW = (7, 9)  # 7 x 9 x 3 = 189 elements per image: image starts break 16-byte alignment, the launch ends in a tail
INTERP_HW = (8, 10)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
FLIP3 = (0, 1, 0)

# integer geometry, step 1: (y0, x0) of the 7 x 9 box
INT_INSIDE = ((0, 0), (5, 7), (12, 14))  # pad 0, boxes inside the source (the last flush bottom-right)
INT_PAD4 = ((-4, -4), (0, 0), (HS - 7 + 4, WS - 9 + 4))  # pad 4: offsets -4, 0, +4 -- the border reads black

# interpolated boxes (y0, x0, h, w) -> 8 x 10, and flips
INTERP_BOXES = ((0, 0, 19, 23),    # downscale 19 -> 8, 23 -> 10: flush with all four edges
                (0, 0, 5, 6),      # upscale 5 x 6 -> 8 x 10, flush top and left: taps at -1 are clamped
                (2.5, 1.25, 9.5, 20.5),  # fractional origin
                (3, 4, 11, 13),    # interior, non-integer steps 1.375 and 1.3
                (14, 17, 5, 6))    # upscale, flush bottom and right: taps at Hs, Ws are clamped; as the last
                                   # sample of the batch it reads the source tensor's very last pixel
INTERP_FLIP = (0, 1, 1, 0, 1)


def noise_source(n: int, hs: int = HS, ws: int = WS, seed: int = 7) -> torch.Tensor:
    """uint8 random noise [n, hs, ws, 3]: neighbouring pixels differ by up to 255, so a half-pixel or tap error
    is of order 1 after normalisation."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, hs, ws, 3), generator=g, dtype=torch.uint8)


def scale_bias64():
    """The fp32 coefficients the op uses (float64 arithmetic, one rounding to fp32), as float64 numpy."""
    mean, std = np.asarray(MEAN, np.float64), np.asarray(STD, np.float64)
    scale, bias = (1.0 / (255.0 * std)).astype(np.float32), (-mean / std).astype(np.float32)
    return scale.astype(np.float64), bias.astype(np.float64)


def int_geom(offsets) -> torch.Tensor:
    return torch.tensor([[y, x, 1.0, 1.0] for y, x in offsets], dtype=torch.float32)


def expected_int(src: torch.Tensor, offsets, flips, out_hw, pad: int) -> np.ndarray:
    """Integer geometry: float32(float64(byte) * float64(scale) + float64(bias)) [N, Ho, Wo, 3]. The float64
    expression is exact (8-bit byte x 24-bit scale, plus a 24-bit bias: fewer than 40 significant bits), so its
    one rounding to fp32 is the fmaf result. Built by slicing a black-padded copy, not by sampling."""
    s = src.numpy()
    n, hs, ws, _ = s.shape
    ho, wo = out_hw
    padded = np.zeros((n, hs + 2 * pad, ws + 2 * pad, 3), np.uint8)
    padded[:, pad:pad + hs, pad:pad + ws] = s
    scale, bias = scale_bias64()
    out = np.empty((n, ho, wo, 3), np.float32)
    for i, ((y0, x0), f) in enumerate(zip(offsets, flips)):
        crop = padded[i, y0 + pad:y0 + pad + ho, x0 + pad:x0 + pad + wo]
        assert crop.shape == (ho, wo, 3), "box outside the padded source"
        if f:
            crop = crop[:, ::-1]
        out[i] = (crop.astype(np.float64) * scale + bias).astype(np.float32)
    return out


def oracle(src: torch.Tensor, geom: torch.Tensor, flip, out_hw, pad: int) -> np.ndarray:
    """The definition in float64 from the fp32 ``geom`` values: float64 [N, Ho, Wo, 3]."""
    s = src.numpy().astype(np.float64)
    n, hs, ws, _ = s.shape
    ho, wo = out_hw
    scale, bias = scale_bias64()
    gm = geom.numpy().astype(np.float64)
    out = np.empty((n, ho, wo, 3), np.float64)

    def taps(coord, size):
        t = np.floor(coord)
        frac = coord - t
        res = []
        for tap in (t, t + 1):
            tap = np.clip(tap, -pad, size - 1 + pad).astype(np.int64)
            inside = (tap >= 0) & (tap < size)
            res.append((np.clip(tap, 0, size - 1), inside.astype(np.float64)))
        return res, frac

    for i in range(n):
        y0, x0, sty, stx = gm[i]
        oy, ox = np.arange(ho, dtype=np.float64), np.arange(wo, dtype=np.float64)
        if flip[i]:
            ox = (wo - 1) - ox
        (ya, yb), fy = taps((y0 - 0.5) + (oy + 0.5) * sty, hs)
        (xa, xb), fx = taps((x0 - 0.5) + (ox + 0.5) * stx, ws)
        v = np.zeros((ho, wo, 3), np.float64)
        for (yi, my), wy in ((ya, 1 - fy), (yb, fy)):
            for (xi, mx), wx in ((xa, 1 - fx), (xb, fx)):
                pix = s[i][yi][:, xi] * (my[:, None] * mx[None, :])[..., None]
                v += (wy[:, None] * wx[None, :])[..., None] * pix
        out[i] = v * scale + bias
    return out


def bf16_bits(x32: np.ndarray) -> np.ndarray:
    """Round-to-nearest-even bf16 bit patterns (uint16) of finite fp32 values."""
    b = np.ascontiguousarray(x32, np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def dense(out: torch.Tensor) -> torch.Tensor:
    """The op's logical [N, 3, Ho, Wo] channels-last result as the dense [N, Ho, Wo, 3] array it is in memory."""
    assert out.dim() == 4 and out.shape[1] == 3
    d = out.permute(0, 2, 3, 1)
    assert d.is_contiguous(), "result is not in channels-last memory"
    return d


def bits_of(out: torch.Tensor) -> np.ndarray:
    d = dense(out).cpu()
    if d.dtype == torch.bfloat16:
        return d.view(torch.int16).numpy().view(np.uint16)
    return d.numpy().view(np.uint32)


def assert_bitwise(out: torch.Tensor, want32: np.ndarray) -> None:
    got = bits_of(out)
    want = bf16_bits(want32) if out.dtype == torch.bfloat16 else np.ascontiguousarray(want32).view(np.uint32)
    bad = int((got != want).sum())
    assert bad == 0, f"{bad} of {want.size} elements differ bitwise ({out.dtype})"


def assert_close(out: torch.Tensor, want64: np.ndarray) -> float:
    """fp32: |out - oracle| <= 5e-4; bf16: <= 5e-4 + 2^-8 |oracle|. For sources of at most 256 pixels per side:
    the fp32 sample coordinate (magnitude < 256) carries at most ~2 ulp = 3e-5 of error, noise pixels differ
    by up to 255, two axes -> at most 1.5e-2 pixel units, times the largest scale 1 / (255 * 0.224) = 0.0175
    gives 2.7e-4. A half-pixel or swapped-axis bug gives errors of order 1."""
    got = dense(out).cpu().to(torch.float64).numpy()
    err = np.abs(got - want64)
    tol = 5e-4 + (2.0 ** -8 * np.abs(want64) if out.dtype == torch.bfloat16 else 0.0)
    worst = float((err - tol).max())
    print(f"augment {out.dtype}: max |err| {err.max():.3e}, max (err - tol) {worst:.3e}")
    assert worst <= 0.0, f"max |out - oracle| {err.max():.3e} exceeds the tolerance by {worst:.3e}"
    return float(err.max())


def interp_geom() -> torch.Tensor:
    from distributed_learning_amd.ops.augment import boxes_to_geom

    y0, x0, h, w = zip(*INTERP_BOXES)
    return boxes_to_geom(torch.tensor(y0), torch.tensor(x0), torch.tensor(h), torch.tensor(w), INTERP_HW)
