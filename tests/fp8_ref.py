"""The FP8 token format of a stored library (include/made_hip.h, "FP8 token storage"), restated with torch's own CPU conversion to
float8_e4m3fn and `frexp` -- nothing here shares code with mgsv_amd/csrc/fp8_format.h or with the numpy formulation in
mgsv_amd/library.py, both of which work on the bit patterns in integer arithmetic.

A token row is D bf16 values, finite and at most MAX_TOKEN = 247 * 2^120 in magnitude: the few bf16 values above it (from
248 * 2^120 = 0x7F78 on) scale to more than 248 and round to the payload 256, which widens to 2^128 -- past the bf16 range.  The
library refuses them with the non-finite ones; "every finite bf16 value" below means every value up to MAX_TOKEN.  e (int8, one per row): 0 for a row of zeros, else the smallest integer with amax * 2^-e <= 448,
clamped to [-120, 120].  Payload: e4m3fn(x * 2^-e), round to nearest even (the product is exact in f32).  Value: bf16(q) * 2^e,
exact."""
import numpy as np
import torch


MAX_TOKEN = 247 * 2.0 ** 120             # 0x7F77, the largest bf16 the format holds
MAX_TOKEN_BITS = 0x7F77


def bf16(bits) -> torch.Tensor:
    """a bf16 tensor of uint16 patterns"""
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint16).view(np.int16)).view(torch.bfloat16)


def bits(t: torch.Tensor) -> np.ndarray:
    """the uint16 patterns of a bf16 tensor"""
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def pow2(e: torch.Tensor) -> torch.Tensor:
    """2^e as f32 for integer e in [-126, 127], from the exponent field (no transcendental function)"""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


def exponent(x: torch.Tensor) -> torch.Tensor:
    """int8 [...]: the exponent of every row of x [..., D] (bf16, finite): amax = m * 2^ex with m in [0.5, 1) -> ex - 9 if
    m <= 0.875 else ex - 8, clamped to [-120, 120]; 0 for a row of zeros"""
    amax = x.float().abs().amax(dim=-1)
    m, ex = torch.frexp(amax)
    e = torch.where(m <= 0.875, ex - 9, ex - 8).clamp(-120, 120)
    return torch.where(amax == 0, torch.zeros_like(e), e).to(torch.int8)


def quantize(x: torch.Tensor):
    """(payload uint8 [..., D], exponent int8 [...]) of bf16 rows x [..., D]"""
    assert x.dtype == torch.bfloat16 and bool((x.float().abs() <= MAX_TOKEN).all())
    e = exponent(x)
    scaled = x.float() * pow2(-e.to(torch.int32)).unsqueeze(-1)     # exact: a power-of-two scaling of an 8-bit significand
    return scaled.to(torch.float8_e4m3fn).view(torch.uint8), e


def dequantize(q: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """bf16 [..., D]: bf16(q) * 2^e; the f32 product is exact and so is its conversion (asserted)"""
    e32 = e.to(torch.int32).unsqueeze(-1)
    half = torch.div(e32, 2, rounding_mode="floor")                 # (2^-129 is no f32 normal: scale in two exact steps)
    wide = q.view(torch.float8_e4m3fn).float() * pow2(half) * pow2(e32 - half)
    out = wide.to(torch.bfloat16)
    assert torch.equal(out.float(), wide), "dequantisation must be exact in bf16"
    return out


def assert_requantized(q, e, q2, e2) -> None:
    """(q2, e2) = quantize(dequantize(q, e)) against (q, e), exactly.  The round trip reproduces payload and exponent for every row
    but two kinds, which keep their VALUES bit for bit and change their encoding:
      * a row whose scaled maximum lies in (224, 232] rounds to the payload 224 (0x76); its dequantised maximum is 448 * 2^(e - 1),
        and the exponent rule -- the SMALLEST e with amax * 2^-e <= 448 -- then gives e - 1 with every payload doubled (exact:
        nothing in the row exceeds 224).  At the clamp (e == -120) such a row keeps both.
      * a row at the clamp whose every value is below 2^-10 * 2^-120 holds zero payloads only: it comes back as a row of zeros,
        whose exponent is 0 by definition.
    Every other row must come back identical."""
    top = (q & 0x7F).amax(dim=-1)
    drops = (top == 0x76) & (e > -120)
    vanish = (top == 0) & (e != 0)
    same = ~drops & ~vanish
    assert torch.equal(e2[same], e[same]) and torch.equal(q2[same], q[same])
    assert bool((e2[vanish] == 0).all()) and bool((e[vanish] == -120).all()) and torch.equal(q2[vanish], q[vanish])
    assert torch.equal(e2[drops].to(torch.int32), e[drops].to(torch.int32) - 1)
    assert bool(((q2[drops] & 0x7F).amax(dim=-1) == 0x7E).all())   # 224 * 2 = 448
    assert torch.equal(dequantize(q2[drops], e2[drops]), dequantize(q[drops], e[drops]))


def special_rows(D: int, j: int = 3) -> torch.Tensor:
    """bf16 [14, D]: the planted rows of the kernel tests -- all zero; one non-zero element in the first / the last lane's fragment;
    amax exactly 448 * 2^j and the next bf16 above it (the m <= 0.875 boundary); exact ties under amax in [256, 448] (17 -> 16,
    19 -> 20, and negative); the subnormal range |x * 2^-e| < 2^-6 with a tie at 2^-10; amax below 448 * 2^-120 (the clamp), a bf16
    subnormal among them; -0; the largest bf16 the format holds."""
    g = torch.Generator().manual_seed(D + j)
    rows = torch.zeros(14, D, dtype=torch.float32)
    rows[1, 3] = 1.5
    rows[2, D - 1] = -0.3
    small = torch.rand(D, generator=g) * 2.0 ** j
    rows[3] = small; rows[3, 5] = 448.0 * 2.0 ** j
    rows[4] = small; rows[4, D - 2] = 450.0 * 2.0 ** j             # 450 = 1.7578125 * 256: the next bf16 above 448 (m = 0.87890625)
    rows[5, :8] = torch.tensor([300.0, 17.0, 19.0, -17.0, -19.0, 18.0, 21.0, 23.0])      # e = 0, quantum 2 in [16, 32)
    rows[6, :8] = torch.tensor([448.0, 2.0 ** -10, 3 * 2.0 ** -10, -2.0 ** -10, 2.0 ** -9, 2.0 ** -7, 5 * 2.0 ** -10, 2.0 ** -11])      # e = 0, subnormals
    rows[7] = torch.randn(D, generator=g) * 2.0 ** -128            # amax < 448 * 2^-120: e = -120, every payload subnormal or tiny
    rows[8, :4] = torch.tensor([2.0 ** -133, 3 * 2.0 ** -133, -2.0 ** -130, 2.0 ** -126])      # bf16 subnormals
    rows[9, :3] = torch.tensor([-0.0, 1.0, -0.0])
    rows[10, 0] = -0.0                                              # amax == 0 with a sign bit set
    rows[11] = torch.randn(D, generator=g); rows[11, 7] = MAX_TOKEN                    # e = 120
    rows[12] = torch.randn(D, generator=g) * 2.0 ** 20
    rows[13] = torch.randn(D, generator=g) * 2.0 ** -20
    out = rows.to(torch.bfloat16)
    assert float(out[4, D - 2]) == 450.0 * 2.0 ** j and float(out[3, 5]) == 448.0 * 2.0 ** j
    return out


def random_rows(R: int, D: int, seed: int) -> torch.Tensor:
    """bf16 [R, D]: normal rows at scales 2^-20 .. 2^20, one scale per row"""
    g = torch.Generator().manual_seed(seed)
    scale = 2.0 ** torch.randint(-20, 21, (R, 1), generator=g).float()
    return (torch.randn(R, D, generator=g) * scale).to(torch.bfloat16)


def kernel_rows(R: int, D: int, seed: int) -> torch.Tensor:
    """bf16 [R, D]: random rows with the planted rows at the front (as many as fit)"""
    x = random_rows(R, D, seed)
    sp = special_rows(D)
    n = min(R, len(sp))
    x[:n] = sp[:n] if R >= len(sp) else sp[[5, 6, 3, 4, 7, 0, 9][:n]]
    return x
