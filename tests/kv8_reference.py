"""Reference side of the fp8 KV-cache forward (include/flashattn_amd_kv8.h): the OCP e4m3fn format from its definition, and the quantiser the
tests fill their caches with.  tests/test_kv8_host.py pins dequant() to torch's own conversion on all 256 codes."""
import numpy as np
import torch

FP8_MAX = 448.0   # the largest finite e4m3fn value: S.1111.110 = 1.75 * 2^8
NAN_CODES = (0x7F, 0xFF)


def _decode(code: int) -> float:
    """1 sign, 4 exponent (bias 7), 3 mantissa bits; no infinities; S.1111.111 is NaN; exponent 0: subnormal, mantissa / 8 * 2^-6"""
    sign = -1.0 if code & 0x80 else 1.0
    e, m = (code >> 3) & 0xF, code & 0x7
    if e == 0xF and m == 0x7:
        return float("nan")
    if e == 0:
        return sign * (m / 8.0) * 2.0 ** -6
    return sign * (1.0 + m / 8.0) * 2.0 ** (e - 7)


TABLE = np.array([_decode(c) for c in range(256)], dtype=np.float64)


def dequant(codes):
    """uint8 array (or a torch.uint8 / torch.float8_e4m3fn tensor) -> float64 array of the values the codes stand for"""
    if isinstance(codes, torch.Tensor):
        codes = (codes.view(torch.uint8) if codes.dtype != torch.uint8 else codes).cpu().numpy()
    return TABLE[np.asarray(codes, dtype=np.uint8)]


def quantize(x, scale: float) -> torch.Tensor:
    """x (array or tensor) -> torch.float8_e4m3fn (CPU): x / scale, clamped to +-448, rounded by torch's cast"""
    t = torch.as_tensor(np.asarray(x, dtype=np.float32) if not isinstance(x, torch.Tensor) else x.float().cpu())
    return (t / scale).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn)
