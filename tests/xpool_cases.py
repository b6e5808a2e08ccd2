"""Named cases of the X-Pool parity suite (tests/test_xpool_parity_gpu.py) and their float64 references.

Shared by tests/test_xpool_dispatch_cpu.py (every case hits the structure it claims: the plan functions of the library and plain
arithmetic on its masks) and the GPU file (every kernel within its bound of chain64 on every case).  A case names a FEW distinct tracks
(`specs`: one mask each) and lays them out along the launch (`order`: distinct track of every position), so the reference of a
2100-track launch costs what fourteen tracks cost; `dead` positions get an all-zero mask on top.  `env`: the measurement knobs the case runs
under; `claim`: what the plan function must answer under them.

Mask specs: int L = the first L segments; "full"; ("holes", L, seed) = a prefix with random holes, first and last kept; ("from", a, L) =
segments [a, L); "last" = only the last segment; ("zeroword", L) = a prefix whose segments [32, 64) are all masked; ("vals", L) = a
prefix whose valid entries hold 0.5 / -1.0 and whose masked entries hold -0.0.
"""
import math
from dataclasses import dataclass, field
from typing import Optional

import torch

import xpool_ref as R

SENT = -7.0                       # sentinel of f32 outputs
SENT_BF = 123.0                   # of bf16 outputs (exact in bf16)
PREFIX96 = (1, 31, 32, 33, 63, 64, 65, 95, 96)
PREFIX512 = (127, 128, 129, 160, 511, 512)
EDGES96 = (("holes", 96, 1), ("from", 5, 70), "last", ("zeroword", 96), ("vals", 50), "full")
VIDEOS = (1, 31, 32, 33, 63, 64, 65, 97)
GAPS = (0, 1, 126, 127, 128, 254, 255, 300)


@dataclass(frozen=True)
class Case:
    name: str
    kernel: str                   # "sims" | "fused" | "pairs" | "attn" | "inbatch"
    Nv: int
    S: int
    specs: tuple                  # masks of the distinct tracks
    D: int = 256
    order: Optional[tuple] = None          # position -> distinct track (None: identity)
    dead: tuple = ()
    no_mask: bool = False
    env: tuple = ()               # ((name, value), ...)
    claim: tuple = ()             # ((field of XpoolPlan, value), ...)
    tiles: tuple = ()             # claimed 32-segment tile counts of the positions, in order
    offset: float = 0.0           # value rows share an offset of this many sigma
    normalize: bool = True        # attn
    out_f32: bool = False         # inbatch
    gaps: tuple = ()              # inbatch: score gap (log2 units, video 0) between the two tiles of distinct track i
    seed: int = 0
    what: str = ""

    @property
    def positions(self):
        return self.order if self.order is not None else tuple(range(len(self.specs)))

    @property
    def Nm(self):
        return len(self.positions)


def mask_of(spec, S):
    m = torch.zeros(S)
    if spec == "full":
        m[:] = 1
    elif spec == "last":
        m[S - 1] = 1
    elif isinstance(spec, int):
        m[:spec] = 1
    elif spec[0] == "holes":
        g = torch.Generator().manual_seed(spec[2])
        m[:spec[1]] = (torch.rand(spec[1], generator=g) > 0.3).float()
        m[0] = 1
        m[spec[1] - 1] = 1
    elif spec[0] == "from":
        m[spec[1]:spec[2]] = 1
    elif spec[0] == "zeroword":
        m[:spec[1]] = 1
        m[32:64] = 0
    elif spec[0] == "vals":
        m[:] = -0.0
        m[:spec[1]:2] = 0.5
        m[1:spec[1]:2] = -1.0
    else:
        raise ValueError(spec)
    return m


def tiles_of(mask_row):
    nz = (mask_row != 0).nonzero()
    return 1 if nz.numel() == 0 else int(nz.max()) // 32 + 1


def _mod(n, k):
    return tuple(i % k for i in range(n))


# ------------------------------------------------------------------------------------------------------------------------ the table
def _sims_cases():
    ten = (96, 1, 33, 64, ("holes", 80, 3), 17, 65, ("from", 40, 96), 32, 95)
    c = [
        Case("sims_prefix", "sims", 33, 96, PREFIX96, env=(("MADE_XPOOL_SIMS_PER", "3"),), claim=(("tracks_per_chunk", 3), ("chunks", 3), ("xcd_order", False)),
             tiles=(1, 1, 1, 2, 2, 2, 3, 3, 3), what="every prefix length at a tile boundary +- 1, three chunks of three tracks"),
        Case("sims_edges", "sims", 64, 96, EDGES96, env=(("MADE_XPOOL_SIMS_PER", "2"),), claim=(("tracks_per_chunk", 2), ("chunks", 3)),
             what="holes, first valid != 0, only the last segment, an all-zero word between live ones, mask values 0.5 / -1.0 / -0.0"),
        Case("sims_nomask", "sims", 31, 40, ("full",) * 4, no_mask=True, env=(("MADE_XPOOL_SIMS_PER", "4"),), claim=(("tracks_per_chunk", 4), ("chunks", 1)),
             what="key_mask = NULL, S no multiple of 16"),
        Case("sims_s64", "sims", 32, 64, (64, 33, 17, 1), env=(("MADE_XPOOL_SIMS_PER", "8"),), claim=(("chunks", 1), ("chunks_launched", 1)), tiles=(2, 2, 1, 1),
             what="two K tiles; one chunk"),
        Case("sims_short_last", "sims", 65, 96, ten, order=_mod(7, 10), env=(("MADE_XPOOL_SIMS_PER", "3"),),
             claim=(("tracks_per_chunk", 3), ("chunks", 3), ("chunks_launched", 3), ("xcd_order", False)), what="Nm = 3 * 2 + 1: the last chunk holds one track"),
        Case("sims_8chunks", "sims", 65, 96, ten, order=_mod(16, 10), env=(("MADE_XPOOL_SIMS_PER", "2"),),
             claim=(("tracks_per_chunk", 2), ("chunks", 8), ("chunks_launched", 8), ("xcd_order", True)), what="exactly eight chunks: the XCD order without padding"),
        Case("sims_9of16_per2", "sims", 65, 96, ten, order=_mod(17, 10), env=(("MADE_XPOOL_SIMS_PER", "2"),),
             claim=(("tracks_per_chunk", 2), ("chunks", 9), ("chunks_launched", 16), ("xcd_order", True)), what="nine chunks padded to sixteen, short last chunk"),
        Case("sims_9of16_per3", "sims", 33, 96, ten, order=_mod(26, 10), env=(("MADE_XPOOL_SIMS_PER", "3"),),
             claim=(("tracks_per_chunk", 3), ("chunks", 9), ("chunks_launched", 16), ("xcd_order", True)), what="nine chunks padded to sixteen"),
        Case("sims_17of24_per3", "sims", 64, 96, ten, order=_mod(50, 10), env=(("MADE_XPOOL_SIMS_PER", "3"),),
             claim=(("tracks_per_chunk", 3), ("chunks", 17), ("chunks_launched", 24), ("xcd_order", True)), what="seventeen chunks padded to twenty-four"),
        Case("sims_default_513", "sims", 33, 32, (32, 1, 31, 17, ("holes", 32, 5), 32, ("from", 9, 20), "last", 2), order=_mod(513, 9),
             claim=(("tracks_per_chunk", 13), ("chunks", 40), ("chunks_launched", 40), ("xcd_order", True)),
             what="no knob: the default chunking gives multi-track chunks in XCD order, one K tile"),
        Case("sims_dead", "sims", 33, 96, ten[:9], dead=(0, 4, 8), env=(("MADE_XPOOL_SIMS_PER", "3"),), claim=(("tracks_per_chunk", 3), ("chunks", 3)),
             what="a dead track first, in the middle and last in a chunk"),
    ]
    c += [Case("sims_nv%d" % nv, "sims", nv, 40, (40, 17, 33), what="ragged video tiles") for nv in VIDEOS]
    c += [Case("sims_offset%d" % o, "sims", 64, 40, (40, 1, 31, 32, 33, ("holes", 40, 2), 17, 39, 8), offset=float(o), seed=o,
               what="value rows share an offset of %d sigma" % o) for o in (1, 4)]
    return c


def _fused_cases():
    twelve = (96, 1, 33, 64, ("holes", 80, 3), 17, 65, ("from", 40, 96), 32, 95, 2, 31)
    c = [
        Case("fused_prefix96", "fused", 33, 96, PREFIX96, env=(("MADE_XPOOL_FUSED_PER", "5"),), claim=(("tracks_per_chunk", 5), ("chunks", 2)),
             tiles=(1, 1, 1, 2, 2, 2, 3, 3, 3), what="every prefix length at a tile boundary +- 1; chunks of five and four tracks"),
        Case("fused_prefix512", "fused", 33, 512, PREFIX512, env=(("MADE_XPOOL_FUSED_PER", "3"),), claim=(("tracks_per_chunk", 3), ("chunks", 2)),
             tiles=(4, 4, 5, 5, 16, 16), what="prefix lengths around 128, 160, 512"),
        Case("fused_s1024", "fused", 33, 1024, (1024, 1, 993, 33), env=(("MADE_XPOOL_FUSED_PER", "4"),), claim=(("tracks_per_chunk", 4), ("chunks", 1)),
             tiles=(32, 1, 32, 2), what="XS_MAX: 32 -> 1 -> 32 -> 2 tiles in one chunk"),
        Case("fused_tile_steps", "fused", 64, 128, (128, 1, 20, 128, 7, 30), env=(("MADE_XPOOL_FUSED_PER", "6"),), claim=(("tracks_per_chunk", 6), ("chunks", 1)),
             tiles=(4, 1, 1, 4, 1, 1), what="consecutive tile counts 4 -> 1, 1 -> 1 (the late path), 1 -> 4; a chunk of six"),
        Case("fused_edges", "fused", 64, 96, EDGES96, env=(("MADE_XPOOL_FUSED_PER", "2"),), claim=(("tracks_per_chunk", 2), ("chunks", 3)),
             what="holes, first valid != 0, only the last segment, an all-zero word, mask values; chunks of two"),
        Case("fused_nomask", "fused", 31, 80, ("full",) * 4, no_mask=True, env=(("MADE_XPOOL_FUSED_PER", "2"),), claim=(("tracks_per_chunk", 2), ("chunks", 2)),
             tiles=(3, 3, 3, 3), what="key_mask = NULL on multi-tile tracks"),
        Case("fused_per1", "fused", 65, 96, twelve, claim=(("tracks_per_chunk", 1), ("chunks", 12)), what="no knob at a small launch: one track per chunk"),
        Case("fused_per5", "fused", 65, 96, twelve, env=(("MADE_XPOOL_FUSED_PER", "5"),), claim=(("tracks_per_chunk", 5), ("chunks", 3)),
             what="chunks of 5, 5, 2: both partial-sum buffers, odd count"),
        Case("fused_per6", "fused", 65, 96, twelve, env=(("MADE_XPOOL_FUSED_PER", "6"),), claim=(("tracks_per_chunk", 6), ("chunks", 2)), what="chunks of 6, 6"),
        Case("fused_dead", "fused", 33, 96, twelve[:9], dead=(0, 4, 8), env=(("MADE_XPOOL_FUSED_PER", "3"),), claim=(("tracks_per_chunk", 3), ("chunks", 3)),
             what="a dead track first, in the middle and last in a chunk"),
        Case("fused_natural", "fused", 33, 17, (17, 1, 16, 9, ("holes", 17, 4), 17, ("from", 3, 12), "last", 2, 17, 5, 13, 17, 11), order=_mod(2100, 14),
             claim=(("tracks_per_chunk", 3), ("chunks", 700)), what="no knob: ceil(Nv / 64) * Nm > 2048 gives three tracks per chunk"),
    ]
    c += [Case("fused_nv%d" % nv, "fused", nv, 40, (40, 17, 33), what="ragged video tiles") for nv in VIDEOS]
    c += [Case("fused_offset%d" % o, "fused", 64, 40, (40, 1, 31, 32, 33, ("holes", 40, 2), 17, 39, 8), offset=float(o), seed=o,
               what="value rows share an offset of %d sigma" % o) for o in (1, 4)]
    return c


def _attn_cases():
    c = [
        Case("attn_prefix96_d256", "attn", 33, 96, PREFIX96, env=(("MADE_XPOOL_ATTN_PER", "3"),), claim=(("tracks_per_chunk", 3), ("chunks", 3)),
             tiles=(1, 1, 1, 2, 2, 2, 3, 3, 3), what="every prefix length; chunks of three tracks: Q stays in registers across them"),
        Case("attn_prefix512_d512", "attn", 65, 512, PREFIX512, D=512, env=(("MADE_XPOOL_ATTN_PER", "3"),), claim=(("tracks_per_chunk", 3), ("chunks", 2), ("video_tiles", 2)),
             tiles=(4, 4, 5, 5, 16, 16), what="4, 5 (one wave holds two tiles) and 16 tiles; Nv = 65: the second video tile is one row"),
        Case("attn_prefix512_d256_raw", "attn", 65, 512, PREFIX512, normalize=False, env=(("MADE_XPOOL_ATTN_PER", "3"),), claim=(("tracks_per_chunk", 3), ("chunks", 2)),
             tiles=(4, 4, 5, 5, 16, 16), what="the same at D = 256 without the normalisation"),
        Case("attn_tiles_d512_raw", "attn", 33, 160, (32, 64, 128, 160), D=512, normalize=False, claim=(("tracks_per_chunk", 1), ("chunks", 4)), tiles=(1, 2, 4, 5),
             what="tile counts 1, 2, 4, 5; no knob: one track per chunk"),
        Case("attn_edges_d256", "attn", 64, 96, EDGES96, env=(("MADE_XPOOL_ATTN_PER", "3"),), claim=(("tracks_per_chunk", 3), ("chunks", 2)), what="mask edges"),
        Case("attn_edges_d512", "attn", 64, 96, EDGES96, D=512, what="mask edges at D = 512"),
        Case("attn_nomask_d256", "attn", 31, 80, ("full",) * 3, no_mask=True, normalize=False, env=(("MADE_XPOOL_ATTN_PER", "3"),), claim=(("chunks", 1),), what="key_mask = NULL"),
        Case("attn_nomask_d512", "attn", 31, 48, ("full",) * 3, no_mask=True, D=512, what="key_mask = NULL, S no multiple of 32"),
        Case("attn_dead_d256", "attn", 33, 96, PREFIX96, dead=(0, 4, 8), env=(("MADE_XPOOL_ATTN_PER", "3"),), claim=(("tracks_per_chunk", 3), ("chunks", 3)),
             what="a dead track first, in the middle and last in a chunk"),
        Case("attn_dead_d512_raw", "attn", 33, 96, PREFIX96, D=512, normalize=False, dead=(0, 4, 8), env=(("MADE_XPOOL_ATTN_PER", "3"),),
             claim=(("tracks_per_chunk", 3), ("chunks", 3)), what="the same at D = 512 without the normalisation"),
        Case("attn_natural", "attn", 65, 33, (33, 1, 32, ("holes", 33, 7), 17), order=_mod(1025, 5), claim=(("tracks_per_chunk", 3), ("chunks", 342), ("video_tiles", 2)),
             what="no knob: Nm > 1024 / ceil(Nv / 64) gives three tracks per chunk"),
    ]
    c += [Case("attn_nv%d" % nv, "attn", nv, 40, (40, 17, 33), D=256 if i % 2 == 0 else 512, normalize=i % 2 == 0, what="ragged video tiles")
          for i, nv in enumerate(VIDEOS)]
    return c


def _inbatch_cases():
    c = []
    for i, S in enumerate((128, 129, 385, 512)):
        for D in (256, 512):
            c.append(Case("inbatch_s%d_d%d" % (S, D), "inbatch", 64 if D == 256 else 33, S, (S, S - 1, ("holes", S, S), ("from", 3, S // 2), 1), D=D,
                          out_f32=(i + D // 256) % 2 == 0, what="%d slice(s) of 128 segments" % ((S + 127) // 128)))
    c += [
        Case("inbatch_prefix512", "inbatch", 37, 512, PREFIX96 + PREFIX512, what="every prefix length"),
        Case("inbatch_edges_d256", "inbatch", 64, 96, EDGES96, what="mask edges (Tpad = 4 for three tiles)"),
        Case("inbatch_edges_d512", "inbatch", 40, 96, EDGES96, D=512, out_f32=True, what="mask edges at D = 512, f32 rows"),
        Case("inbatch_nomask", "inbatch", 31, 200, ("full",) * 3, no_mask=True, what="key_mask = NULL, S no multiple of 32"),
        Case("inbatch_dead", "inbatch", 33, 160, (160, 33, 64, 1, 129), dead=(0, 2, 4), out_f32=True, what="dead tracks first, in the middle and last"),
        Case("inbatch_gaps_d256", "inbatch", 33, 64, ("full",) * len(GAPS), gaps=GAPS, out_f32=True,
             what="score gaps of 0 .. 300 log2 units between a track's two tiles: the exponent-field subtraction and its clamp at 255"),
        Case("inbatch_gaps_d512", "inbatch", 64, 64, ("full",) * len(GAPS), D=512, gaps=GAPS, what="the same at D = 512, bf16 rows"),
    ]
    c += [Case("inbatch_nv%d" % nv, "inbatch", nv, 140, (140, 17, 129), D=256 if i % 2 == 0 else 512, out_f32=i % 3 == 0, what="fewer than 64 videos")
          for i, nv in enumerate(v for v in VIDEOS if v <= 64)]
    return c


def _pairs_cases():
    return [
        Case("pairs_ranges", "pairs", 40, 96, (96, 33, ("holes", 80, 3), 65, 17, 64), dead=(5,),
             what="ranges of 0, 1, 32, 33, 65 and 5 pairs (the last on a dead track); videos unordered and repeated; indices -1 and Nv; start values to clamp"),
        Case("pairs_prefix", "pairs", 33, 96, PREFIX96, what="every prefix length, three pairs each"),
        Case("pairs_edges", "pairs", 64, 96, EDGES96, what="mask edges, 40 pairs each (two tiles)"),
        Case("pairs_nomask", "pairs", 31, 40, ("full",) * 3, no_mask=True, what="key_mask = NULL, S no multiple of 16"),
    ] + [Case("pairs_offset%d" % o, "pairs", 64, 40, (40, 1, 31, 32, 33, ("holes", 40, 2), 17, 39, 8), offset=float(o), seed=o,
              what="value rows share an offset of %d sigma" % o) for o in (1, 4)]


CASES = _sims_cases() + _fused_cases() + _attn_cases() + _inbatch_cases() + _pairs_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
SCORING = ("sims", "fused", "pairs")
PAIR_COUNTS = {"pairs_ranges": (0, 1, 32, 33, 65, 5), "pairs_prefix": (3,) * 9, "pairs_edges": (40,) * 6, "pairs_nomask": (7, 33, 1)}


# ------------------------------------------------------------------------------------------------------------------------ operands
@dataclass
class Built:
    case: Case
    Q: torch.Tensor               # [Nv, D] float32, bf16-representable
    K: torch.Tensor               # distinct tracks [Nd, S, D]
    U: torch.Tensor               # [Nd, S, D]        (sims / pairs: UU [Nd, S, 2 D])
    mask: torch.Tensor            # distinct masks [Nd, S] (values as the kernel gets them)
    par: dict = field(default_factory=dict)       # ln2, Wl, bl, ln3, av, bv, vn
    pairs: Optional[tuple] = None                 # (start int32 [U + 1] with values to clamp, video int32 [P], P)

    @property
    def valid(self):
        return self.mask != 0

    def launch_mask(self, with_dead=True):
        """[Nm, S] mask of the launch (None for a no-mask case)"""
        if self.case.no_mask:
            return None
        m = self.mask[list(self.case.positions)].clone()
        if with_dead:
            for p in self.case.dead:
                m[p] = 0
        return m


def _rn(g, *shape):
    return torch.randn(*shape, generator=g)


def build(case: Case) -> Built:
    g = torch.Generator().manual_seed(1000 + case.seed + 7 * len(case.specs) + case.Nv)
    D, S, Nd, Nv = case.D, case.S, len(case.specs), case.Nv
    Q = R.bf(_rn(g, Nv, D))
    K = R.bf(_rn(g, Nd, S, D))
    U = R.bf(_rn(g, Nd, S, D) + case.offset)
    mask = torch.stack([mask_of(sp, S) for sp in case.specs])
    b = Built(case, Q, K, U, mask)
    scale = R.scale_of(D)
    if case.gaps:
        # tile B (the other tile) holds small scores; one row of tile A is beta q_0, beta searched so that video 0's tile references differ by the gap
        K = R.bf(K * 0.25)
        unit = float((Q[0].double() ** 2).sum()) * scale * R.LOG2E
        for i, gap in enumerate(case.gaps):
            ta = i % 2                                            # the tile that holds the spike
            seg = 32 * ta + 5
            sB = (K[i, 32 * (1 - ta):32 * (2 - ta)].double() @ Q[0].double()) * scale * R.LOG2E
            refB = math.ceil(float(sB.max()))
            found = False
            for k in range(400):
                beta = (gap + refB - 0.5) / unit * (1.0 + 0.0005 * (k - 200))
                row = R.bf(beta * Q[0])
                Ki = K[i].clone()
                Ki[seg] = row
                sA = (Ki[32 * ta:32 * ta + 32].double() @ Q[0].double()) * scale * R.LOG2E
                mA = float(sA.max())
                if math.ceil(mA) - refB == gap and 0.2 < mA - math.floor(mA) < 0.8:
                    K[i] = Ki
                    found = True
                    break
            assert found, (case.name, gap)
        b.K = K
    if case.kernel in SCORING:
        Wl = R.bf(_rn(g, D, D) / math.sqrt(D))
        ln2 = (1 + 0.1 * _rn(g, D), 0.1 * _rn(g, D))
        ln3 = (1 + 0.1 * _rn(g, D), 0.1 * _rn(g, D))
        bl = 0.1 * _rn(g, D)
        b.par.update(Wl=Wl, ln2=ln2, ln3=ln3, bl=bl)
        if case.kernel in ("sims", "pairs"):
            # the caller's preparation (engine.py): W'' = (W + I) diag(g2) in bf16, b'' = (W + I) b2 + b, W'' 1, u'' = W'' u in bf16
            W64 = Wl.double() + torch.eye(D, dtype=torch.float64)
            W2 = R.bf((W64 * ln2[0].double()[None, :]).float())
            b.par["av"] = (W64 @ ln2[1].double() + bl.double()).float()
            b.par["bv"] = W2.double().sum(1).float()
            b.U = torch.cat([U, R.bf((U.double() @ W2.double().t()).float())], -1)
        # the videos: three of four are a noisy copy of LayerNorm3's row of one of their pairs, so that the similarities span the range
        z3 = z3_64(b)
        live = [i for i in range(Nd) if bool(b.valid[i].any())]
        vn = _rn(g, Nv, D)
        for n in range(Nv):
            if n % 4 != 3:
                z = z3[live[n % len(live)], n]
                vn[n] = z.float() + 0.5 * float(z.std()) * vn[n]
        b.par["vn"] = torch.nn.functional.normalize(vn, dim=-1)
    if case.kernel == "pairs":
        counts = PAIR_COUNTS.get(case.name, (5,) * Nd)
        P = sum(counts)
        video = torch.randint(0, Nv, (P,), generator=g).int()     # unordered, repeated
        start = torch.tensor([0] + list(torch.tensor(counts).cumsum(0)), dtype=torch.int32)
        if case.name == "pairs_ranges":
            video[40] = -1
            video[70] = Nv
            video[-1] = -1
            start[0] = -5                                        # clamped to 0 (range 0 is empty)
            start[-1] = P + 7                                    # clamped to P
        b.pairs = (start, video, P)
    return b


def z3_64(b: Built):
    c, p = b.case, b.par
    scale = R.scale_of(c.D)
    if c.kernel == "fused":
        return R.z3_unfolded64(b.Q, b.K, b.U, b.valid, p["ln2"], p["Wl"], p["bl"], p["ln3"], scale)
    return R.z3_folded64(b.Q, b.K, b.U, b.valid, p["av"], p["bv"], p["ln3"], scale)


def reference(b: Built):
    """(chain64, chain_model) on the DISTINCT tracks: sims [Nv, Nd] for the scoring kernels, rows [Nd, Nv, D] for the others"""
    c, p = b.case, b.par
    scale = R.scale_of(c.D)
    if c.kernel in SCORING:
        ref = R.cosine64(z3_64(b), p["vn"])
        if c.kernel == "fused":
            mod = R.model_fused(b.Q, b.K, b.U, b.valid, p["ln2"], p["Wl"], p["bl"], p["ln3"], p["vn"], scale)
        elif c.kernel == "sims":
            mod = R.model_sims(b.Q, b.K, b.U, b.valid, p["av"], p["bv"], p["ln3"], p["vn"], scale)
        else:
            mod = R.model_pairs(b.Q, b.K, b.U, b.valid, p["av"], p["bv"], p["ln3"], p["vn"], scale)
        return ref, mod
    if c.kernel == "attn":
        return R.rows64(b.Q, b.K, b.U, b.valid, scale, c.normalize), R.model_attention(b.Q, b.K, b.U, b.valid, scale, c.normalize)
    return R.rows64(b.Q, b.K, b.U, b.valid, scale, False), R.model_inbatch(b.Q, b.K, b.U, b.valid, scale, not c.out_f32)


_CACHE = {}


def amplification(case: Case) -> float:
    """How much more the case's value offset lets a rounding error weigh than the same case without it: the ratio of the two model-derived
    bounds (1 for a case without an offset).  y = k1 z + k2 Bv + Av cancels the rows' common part; every rounding in front of it -- the
    model's bf16 ones and the f32 ones in which the 32- and the 64-video kernel of made_xpool_sims differ -- is passed on times this factor."""
    if case.offset == 0:
        return 1.0
    import dataclasses
    twin = dataclasses.replace(case, name=case.name + "_twin", offset=0.0)
    return max(1.0, prepared(case)[2] / prepared(twin)[2])


def prepared(case: Case):
    """(Built, chain64, bound) of a case, computed once per process and never modified"""
    if case.name not in _CACHE:
        b = build(case)
        ref, mod = reference(b)
        live = b.valid.any(1)
        if case.kernel in SCORING:
            bd = R.bound(mod[:, live], ref[:, live])
        else:
            bd = R.bound(mod[live], ref[live])
        _CACHE[case.name] = (b, ref, bd)
    return _CACHE[case.name]
