"""Shared cases of the core-kernel tests (test_core_kernels_gpu.py and
test_core_kernels_reference.py): sizes taken from the compact geometry, data
kinds with planted bit patterns, thresholds, EF triples and Adam states.
Everything is built on the CPU, once per key, and handed out read-only:
callers copy before they let an op write."""
import math

import torch

FLT_MAX = 3.4028234663852886e38
INF = float("inf")

# bit patterns (as signed int32) the kernels must treat by the bit rule
NAN_PAYLOADS = [0x7FC00000, 0xFFC00000 - (1 << 32), 0x7F800001, 0x7FFFFFFF]
SPECIAL_BITS = [
    0x00000000,               # +0
    0x80000000 - (1 << 32),   # -0
    0x7F800000,               # +inf
    0xFF800000 - (1 << 32),   # -inf
    *NAN_PAYLOADS,
    0x00000001,               # smallest subnormal
    0x80000001 - (1 << 32),   # ... negative
    0x007FFFFF,               # largest subnormal
    0x7F7FFFFF,               # FLT_MAX
    0xFF7FFFFF - (1 << 32),   # -FLT_MAX
]


def compact_geom(n):
    """(chunk, nblocks) as bindings.cpp compact_geom picks them: a block owns
    `chunk` elements, each of its 4 waves chunk/4, in steps of 512."""
    unit = 2048
    nchunks = min(max((n + unit - 1) // unit, 1), 2048)
    chunk = ((n + nchunks - 1) // nchunks + unit - 1) // unit * unit
    return chunk, max((n + chunk - 1) // chunk, 1)


SIZES_SMALL = [
    1, 7, 8, 9,          # below / at / above one lane's 8-element run
    63, 64, 65,          # wave width
    511, 512, 513,       # one 512-element wave step
    2047, 2048, 2049,    # one block (4 waves x 512)
    6145,                # four blocks, the last holds one element
    65537,               # mid-size, 33 blocks
    1_000_003,           # mid-size, 489 blocks, odd
]
SIZES_LARGE = [
    4_194_299,  # 2048 blocks: the offset scan runs at its full 8192 entries,
                # ragged tail in the last wave
    4_196_358,  # chunk 4096: two 512-steps per wave, 1025 blocks
    8_390_011,  # chunk 6144: three steps per wave (have_next true, true,
                # false), 1366 blocks, the last block partly empty
]
LARGE_KINDS = ("randn", "edges", "dense")  # the kinds that run SIZES_LARGE
KINDS = ["randn", "quant", "edges", "dense", "special", "subnormal_only",
         "wide", "low_bits", "mid_bits"]


def sizes_for(kind):
    return SIZES_SMALL + (SIZES_LARGE if kind in LARGE_KINDS else [])


def kind_size_params():
    return [(k, n) for k in KINDS for n in sizes_for(k)]


def bits(x):
    """int32 view: equality of these tells -0 from +0 and NaN payloads apart."""
    return x.contiguous().view(torch.int32)


def from_bits(b):
    return b.to(torch.int32).contiguous().view(torch.float32)


def shifted(x):
    """A GPU copy of x whose data pointer is one element off 16-byte
    alignment."""
    buf = torch.empty(x.numel() + 8, dtype=x.dtype, device="cuda")
    view = buf[1:1 + x.numel()]
    view.copy_(x)
    assert view.data_ptr() % 16 != 0
    return view


def _seed(kind, n, salt=0):
    g = torch.Generator()
    g.manual_seed(n * 131 + sum(map(ord, kind)) * 7 + salt)
    return g


# -- planted pattern "edges" -------------------------------------------------

def edges_positions(n):
    """Ascending positions of the non-zeros of the `edges` kind: 0 and n-1,
    every multiple of 512 and the element before it, and 8j +- 1 inside the
    first and the last 512-run."""
    pos = {0, n - 1}
    for m in range(512, n, 512):
        pos.update((m - 1, m))
    last = (n - 1) // 512 * 512
    for lo in {0, last}:
        for j in range(lo, min(lo + 512, n), 8):
            pos.update((j - 1, j + 1))
    lo_ok = sorted(p for p in pos if 0 <= p < n)
    return torch.tensor(lo_ok, dtype=torch.int64)


def edges_expected(n):
    """(idx int32, val) a compaction of `edges` at tau = 0.5 must return, in
    closed form: the planted positions, values alternating +1, -1."""
    pos = edges_positions(n)
    val = torch.where(torch.arange(pos.numel()) % 2 == 0, 1.0, -1.0)
    return pos.to(torch.int32), val.to(torch.float32)


_data = {}


def make(kind, n):
    """The fp32 CPU tensor of (kind, n); cached, do not write to it."""
    key = (kind, n)
    if key in _data:
        return _data[key]
    g = _seed(kind, n)
    if kind == "randn":
        t = torch.randn(n, generator=g)
    elif kind == "quant":
        # multiples of 1/4: tie classes of thousands
        t = torch.round(torch.randn(n, generator=g) * 4.0) / 4.0
    elif kind == "edges":
        t = torch.zeros(n)
        idx, val = edges_expected(n)
        t[idx.long()] = val
    elif kind == "dense":
        # no zero anywhere: at tau < 0 and tau = 0 every lane stores all 8
        # of its elements in every step
        t = torch.randn(n, generator=g)
        t[t == 0] = 1.0
    elif kind == "special":
        t = torch.randn(n, generator=g)
        sp = from_bits(torch.tensor(SPECIAL_BITS, dtype=torch.int64))
        where = (torch.arange(len(SPECIAL_BITS)) * max(1, n // len(SPECIAL_BITS))
                 + min(3, n - 1)) % n
        t[where] = sp
    elif kind == "subnormal_only":
        # |bits| < 2^21: radix level 1 puts everything into bin 0
        b = torch.randint(0, 1 << 21, (n,), generator=g)
        s = torch.randint(0, 2, (n,), generator=g) * (-(1 << 31))
        t = from_bits(b + s)
    elif kind == "wide":
        e = torch.randint(-120, 121, (n,), generator=g)
        t = torch.ldexp(torch.randn(n, generator=g), e)
    elif kind == "low_bits":
        # one exponent and upper mantissa; only the low 10 bits differ, so
        # radix level 3 decides
        b = 0x3F9D5400 + torch.randint(0, 1 << 10, (n,), generator=g)
        s = torch.randint(0, 2, (n,), generator=g) * (-(1 << 31))
        t = from_bits(b + s)
    elif kind == "mid_bits":
        # only the middle 11 bits (10..20) differ: level 2 decides
        b = 0x3F800155 + (torch.randint(0, 1 << 11, (n,), generator=g) << 10)
        s = torch.randint(0, 2, (n,), generator=g) * (-(1 << 31))
        t = from_bits(b + s)
    else:
        raise AssertionError(kind)
    assert t.dtype == torch.float32 and t.numel() == n
    _data[key] = t
    return t


def prev_toward_zero(tau):
    """The fp32 value one bit pattern below tau > 0 (nextafter towards 0)."""
    b = bits(torch.tensor([tau], dtype=torch.float32))
    return float(from_bits(b - 1))


def an_element_magnitude(t):
    """|x| of some element of t that is finite and non-zero (the median of
    those), or None."""
    a = t.abs()
    a = a[torch.isfinite(a) & (a > 0)]
    if a.numel() == 0:
        return None
    return float(a.sort().values[a.numel() // 2])


def thresholds(kind, n):
    """The taus every selection case runs: negative, 0, an element's own
    magnitude (strictly excluded) and the value just below it (included), a
    double that is no fp32 value, FLT_MAX and +inf."""
    taus = [-1.0, 0.0]
    e = an_element_magnitude(make(kind, n))
    if e is not None:
        taus += [e, prev_toward_zero(e)]
    return taus + [0.1, FLT_MAX, INF]


def adaptive_cases(kind, n):
    """(taus, hi_limit, expected pick or None) for compact_adaptive: 1, 4
    and 8 candidates, one of them negative, with the pick at index 0, at a
    middle index whose count equals hi_limit exactly, and at the last index
    by fall-through (no count fits)."""
    from oktopk_amd.ops import reference as R

    t = make(kind, n)
    a = t.abs()
    a = a[torch.isfinite(a)].sort().values
    if a.numel() == 0:
        a = torch.zeros(1)

    def q(f):
        return float(a[min(a.numel() - 1, int(f * a.numel()))])

    t8 = [-1.0, q(0.3), q(0.5), q(0.7), q(0.9), q(0.97), q(0.99), q(0.999)]
    t4 = [-1.0, q(0.5), q(0.9), q(0.99)]
    out = [([q(0.9)], 0, 0), ([-1.0], n, 0)]
    for taus in (t4, t8):
        counts = R.count_multi_gt(t, taus)
        mid = len(taus) // 2
        out.append((taus, n, 0))               # the negative tau fits at once
        out.append((taus, counts[mid], None))  # count == hi_limit exactly
        out.append((taus, -1, len(taus) - 1))  # nothing fits: the last
    return out


# -- error-feedback triples ---------------------------------------------------

EF_KINDS = ["randn", "bf16", "cancel", "infnan", "bf16_edge", "subnormal"]
EF_LARGE_KINDS = ("randn", "bf16")
# every n % 8 in 1..7 occurs; 8 and 6152 have none
EF_SIZES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 517, 2051, 6150, 6152, 65537,
            1_000_003]
EF_SIZES_LARGE = [4_196_358, 8_390_011]


def ef_params():
    return [(k, n) for k in EF_KINDS
            for n in EF_SIZES + (EF_SIZES_LARGE if k in EF_LARGE_KINDS else [])]


_ef = {}


def ef_case(kind, n):
    """(t, residual, grad | None) on the CPU; cached, do not write."""
    key = (kind, n)
    if key in _ef:
        return _ef[key]
    g = _seed("ef" + kind, n)
    grad = None
    if kind == "randn":
        t = torch.randn(n, generator=g)
        r = torch.randn(n, generator=g) * 0.1
    elif kind == "bf16":
        t = torch.full((n,), 123.0)  # stale: must not be read
        grad = torch.randn(n, generator=g).to(torch.bfloat16)
        r = torch.randn(n, generator=g) * 0.1
    elif kind == "cancel":
        # g = -r on two of three elements: the restored value is +0.0
        r = torch.randn(n, generator=g)
        t = torch.where(torch.arange(n) % 3 != 0, -r,
                        torch.randn(n, generator=g))
    elif kind == "infnan":
        # inf + (-inf) restores NaN (selected at every tau); inf + finite
        t = torch.randn(n, generator=g)
        r = torch.randn(n, generator=g) * 0.1
        i = torch.arange(n)
        t[i % 5 == 0] = INF
        r[i % 10 == 0] = -INF
        t[i % 7 == 3] = -INF
    elif kind == "bf16_edge":
        # bf16 -0.0, bf16 subnormals and cancelling bf16 gradients
        t = torch.full((n,), 123.0)
        gb = torch.randn(n, generator=g).to(torch.bfloat16).view(torch.int16)
        i = torch.arange(n)
        gb[i % 4 == 0] = -0x8000                                   # -0.0
        sub = torch.randint(1, 0x80, (n,), generator=g).to(torch.int16)
        gb[i % 4 == 1] = sub[i % 4 == 1]                           # subnormal
        gb[i % 8 == 5] = (sub[i % 8 == 5] - 0x8000).to(torch.int16)
        grad = gb.view(torch.bfloat16)
        r = torch.randn(n, generator=g) * 0.1
        r[i % 8 == 0] = 0.0                       # -0 + +0 = +0
        r[i % 8 == 4] = -0.0                      # -0 + -0 = -0
        r[i % 4 == 1] = from_bits(torch.randint(0, 1 << 20, (n,), generator=g))[i % 4 == 1]
        r[i % 4 == 2] = -grad.float()[i % 4 == 2]  # exact cancellation
    elif kind == "subnormal":
        # both addends subnormal: the sum is subnormal or just normal
        t = from_bits(torch.randint(0, 1 << 23, (n,), generator=g)
                      + torch.randint(0, 2, (n,), generator=g) * (-(1 << 31)))
        r = from_bits(torch.randint(0, 1 << 23, (n,), generator=g)
                      + torch.randint(0, 2, (n,), generator=g) * (-(1 << 31)))
    else:
        raise AssertionError(kind)
    _ef[key] = (t, r, grad)
    return _ef[key]


def ef_restored(kind, n):
    t, r, grad = ef_case(kind, n)
    return (grad.float() if grad is not None else t) + r


def ef_tau_sets(kind, n):
    """[(taus, hi_limit)]: four ascending candidates from the restored
    values' own quantiles with a limit that skips the first, and tau = 0
    with everything allowed (dense stores; +0 sums dropped, NaN kept)."""
    a = ef_restored(kind, n).abs()
    a = a[torch.isfinite(a)].sort().values
    if a.numel() == 0:
        a = torch.zeros(1)

    def q(f):
        return float(a[min(a.numel() - 1, int(f * a.numel()))])

    return [([q(0.5), q(0.9), q(0.99), q(0.999)], n // 20), ([0.0], n)]


# -- Adam states --------------------------------------------------------------

ADAM_SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 100_003, 600_001]
# "exact": every hyperparameter and 1 - b exact in binary
ADAM_HYPER = {
    "exact": dict(lr=2.0 ** -10, b1=0.875, b2=1.0 - 2.0 ** -10, eps=2.0 ** -20),
    "production": dict(lr=2e-4, b1=0.9, b2=0.999, eps=1e-6),
}
ADAM_WD = {"exact": [0.0, 2.0 ** -7], "production": [0.0, 0.01]}
ADAM_GSCALES = [None, 1.0, 0.375]
ADAM_STRETCHES = 7

_adam = {}


def adam_case(n, hyper):
    """(p, g, m, v) fp32 on the CPU for one hyperparameter set.  Element i
    belongs to stretch i % 7, so every stretch occurs at every n >= 7 and
    straddles the float4 loop and the scalar tail:
      0 generic (|p| ~ 1)         1 |p| ~ lr: the 6u*lr term dominates
      2 v = 0                     3 v ~ eps^2
      4 g = 0                     5 m*b1 ~ -c1*g: the m update cancels
      6 m = v = g = 0"""
    key = (n, hyper)
    if key in _adam:
        return _adam[key]
    h = ADAM_HYPER[hyper]
    g_ = _seed("adam" + hyper, n)
    p = torch.randn(n, generator=g_)
    g = torch.randn(n, generator=g_)
    m = torch.randn(n, generator=g_) * 0.1
    v = (torch.randn(n, generator=g_) * 0.1) ** 2
    s = torch.arange(n) % ADAM_STRETCHES
    p[s == 1] *= h["lr"]
    v[s == 2] = 0.0
    v[s == 3] = (h["eps"] ** 2 * (0.5 + 1.5 * torch.rand(n, generator=g_)))[s == 3]
    g[s == 4] = 0.0
    c1 = 1.0 - h["b1"]
    g[s == 5] = (-m * h["b1"] / c1 * (1 + 1e-6 * torch.randn(n, generator=g_)))[s == 5]
    for x in (m, v, g):
        x[s == 6] = 0.0
    _adam[key] = (p, g, m, v)
    return _adam[key]


# crafted master weights for the bf16 mirror (run with lr = 0, wd = 0)
MIRROR_FINITE_BITS = [
    0x3F808000,               # tie, even mantissa below: rounds down
    0x3F818000,               # tie, odd mantissa below: rounds up
    0x3F807FFF, 0x3F808001,   # just below / above a tie
    0xBF808000 - (1 << 32), 0xBF818000 - (1 << 32),
    0x3FFFFFFF,               # rounds up into the next exponent
    0x7F7FFFFF,               # FLT_MAX -> inf
    0xFF7FFFFF - (1 << 32),   # -> -inf
    0x7F7F7FFF,               # largest that stays finite
    0x00000001, 0x007FFFFF, 0x00008000, 0x00018000,  # subnormals
    0x80000001 - (1 << 32),
    0x00000000, 0x80000000 - (1 << 32),              # +-0
]
MIRROR_NONFINITE_BITS = [0x7F800000, 0xFF800000 - (1 << 32), *NAN_PAYLOADS,
                         0x7FFF8000, 0xFFFFFFFF - (1 << 32)]


def f2b_emulated(x):
    """Bit-level emulation of the kernels' adam_f2b in torch integer ops:
    round to nearest even on the bit pattern, NaN kept a NaN (upper 16 bits
    with the quiet bit set).  Returns bf16."""
    u = bits(x).to(torch.int64) & 0xFFFFFFFF
    rne = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    nan = (u >> 16) | 0x0040
    h = torch.where((u & 0x7FFFFFFF) > 0x7F800000, nan, rne)
    h = torch.where(h >= 0x8000, h - 0x10000, h)
    return h.to(torch.int16).view(torch.bfloat16)


def f2b_parent(x):
    """The rounding add alone, without the NaN select: what adam_f2b was."""
    u = bits(x).to(torch.int64) & 0xFFFFFFFF
    h = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    h = torch.where(h >= 0x8000, h - 0x10000, h)
    return h.to(torch.int16).view(torch.bfloat16)


# -- norms ----------------------------------------------------------------------

NORM_SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 100_003, 600_001]
_norm = {}


def norm_case(kind, n):
    """(t fp32, exact sum of squares as a Python number).  `integer`:
    integers in [-1024, 1024], every partial sum of squares is an integer
    below 2^53, exact in fp64 in any order.  `randn`: math.fsum of the
    (exact) fp64 squares."""
    key = (kind, n)
    if key in _norm:
        return _norm[key]
    g = _seed("norm" + kind, n)
    if kind == "integer":
        t = torch.randint(-1024, 1025, (n,), generator=g).float()
        exact = int((t.long() ** 2).sum())
    else:
        t = torch.randn(n, generator=g)
        exact = math.fsum((t.double() ** 2).tolist())
    _norm[key] = (t, exact)
    return _norm[key]
