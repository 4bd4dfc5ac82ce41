"""OCP MXFP4 (Microscaling Formats v1.0): e2m1 elements with one shared e8m0 scale per 32 consecutive elements of a row — the
expert format of ``EngineConfig.mxfp4_slots``.  torch only; CPU or GPU tensors.

A code is 4 bits: sign (bit 3), exponent (bits 2..1), mantissa (bit 0) -> 0, 0.5, 1, 1.5, 2, 3, 4, 6.  Element 2j of a row sits in
the LOW nibble of byte j (torch.float4_e2m1fn_x2's convention).  A scale byte b stands for 2^(b - 127).  Every value
``code x 2^(b - 127)`` has two significant bits, so it is exact in bfloat16 wherever it is a normal bfloat16 number (b >= 2)."""
import torch

E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
BLOCK = 32


def mxfp4_quantize(w: torch.Tensor):
    """w [R, K] (K % 32 == 0, finite) -> (codes uint8 [R, K/2], scales uint8 [R, K/32]) by the OCP MX v1.0 rule: the shared
    exponent of a block is floor(log2(amax)) - 2 (2 = e2m1's largest exponent), clamped to scale bytes 1..254; the elements are
    rounded to nearest-even on the e2m1 grid and saturate at +-6; an all-zero block gets scale byte 127."""
    if w.dim() != 2 or w.shape[1] % BLOCK:
        raise ValueError(f"mxfp4_quantize takes [R, K] with K % {BLOCK} == 0, got {tuple(w.shape)}")
    R, K = w.shape
    x = w.detach().to(torch.float32).reshape(R, K // BLOCK, BLOCK)
    amax = x.abs().amax(dim=-1)
    # floor(log2(amax)) is the fp32 exponent field (frexp: amax = m * 2^e with m in [0.5, 1), so floor(log2) = e - 1); exact,
    # subnormal inputs included
    _, e = torch.frexp(amax)
    b = (e.to(torch.int32) - 1 - 2 + 127).clamp(1, 254)
    b = torch.where(amax == 0, torch.full_like(b, 127), b)
    y = torch.ldexp(x, (127 - b).unsqueeze(-1)).abs()  # |x| / 2^(b - 127), exact (a power of two)
    # round to nearest-even on the grid 0 0.5 1 1.5 | 2 3 | 4 6: steps of 0.5 below 2, of 1 below 4, of 2 above; torch.round rounds
    # halves to even, and "even" on each stretch is the code with mantissa bit 0
    q = torch.where(y < 2, torch.round(y * 2) / 2, torch.where(y < 4, torch.round(y), torch.round(y / 2) * 2)).clamp(max=6.0)
    grid = torch.tensor(E2M1_VALUES, dtype=torch.float32, device=q.device)
    code = torch.bucketize(q, grid).to(torch.uint8)  # q is ON the grid: the index of the equal entry
    code = code | (torch.signbit(x).to(torch.uint8) << 3)
    code = code.reshape(R, K // 2, 2)
    codes = (code[..., 0] | (code[..., 1] << 4)).contiguous()
    return codes, b.to(torch.uint8).contiguous()


def mxfp4_dequantize(codes: torch.Tensor, scales: torch.Tensor, dtype=torch.bfloat16):
    """(codes uint8 [R, K/2], scales uint8 [R, K/32]) -> [R, K] of `dtype`: value(code) x 2^(scale - 127), computed in fp32"""
    if codes.dtype != torch.uint8 or scales.dtype != torch.uint8 or codes.dim() != 2 or scales.dim() != 2:
        raise ValueError("codes and scales must be 2-D uint8 tensors")
    R, K2 = codes.shape
    if scales.shape[0] != R or scales.shape[1] * 16 != K2:
        raise ValueError(f"codes {tuple(codes.shape)} need scales [{R}, {K2 // 16}], got {tuple(scales.shape)}")
    nib = torch.stack((codes & 15, codes >> 4), dim=-1).reshape(R, K2 * 2).to(torch.int64)
    grid = torch.tensor(E2M1_VALUES + tuple(-v for v in E2M1_VALUES), dtype=torch.float32, device=codes.device)
    v = grid[nib].reshape(R, K2 // 16, BLOCK)
    out = torch.ldexp(v, (scales.to(torch.int32) - 127).unsqueeze(-1))
    return out.reshape(R, K2 * 2).to(dtype)
