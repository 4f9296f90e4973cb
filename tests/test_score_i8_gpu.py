"""The int8 operand mode of the MFMA pre-filter (`score_i8`, csrc/score_mfma.h "int8 limbs"): the quantised operands, the
integer product with its fp32 combine and the margin E2 against numpy statements, the int8 arm of the self-check, and the
scoring results end to end -- `score_i8` 1 against 0 against the exact kernels, bit for bit.  Shapes are the smallest at
which this code can go wrong: partial tiles, tiles across video boundaries, a partial query group, one and several groups."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from vfr_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
XMAX = 127 * 65536 + 127 * 256 + 127
U = 2.0 ** -24


@pytest.fixture(scope="module")
def vfr():
    from vfr_amd import _vfr
    _vfr.lib()
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return _vfr


@pytest.fixture(autouse=True)
def prefilter_reachable(vfr):
    """Tiny banks and batches must reach the pre-filter kernels: no few-queries path, no minimum bank size."""
    old = {n: vfr.get_option(n) for n in ("score_smallq", "score_mfma_min", "score_i8")}
    vfr.set_option("score_smallq", 0)
    vfr.set_option("score_mfma_min", 0)
    yield
    for n, v in old.items():
        vfr.set_option(n, v)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bank_of(vfr, V, counts):
    return vfr.VideoBank(dev(V.astype(np.float32)), dev(synth.clip_offsets(np.asarray(counts)).astype(np.int32)))


# ---- numpy statements --------------------------------------------------------------------------------------------------
def quantise(x, s):
    """X = rint(x s) in fp64, clamped to |X| <= XMAX."""
    return np.clip(np.rint(x.astype(np.float64) * s), -XMAX, XMAX).astype(np.int64)


def digits(X):
    """Three balanced base-256 digits in [-128, 127], least significant first."""
    d0 = (X + 128) % 256 - 128
    X1 = (X - d0) // 256
    d1 = (X1 + 128) % 256 - 128
    d2 = (X1 - d1) // 256
    return np.stack([d0, d1, d2], axis=-2)                                  # [..., 3, K]


def planes(x, s):
    """[rows, 3, 128] int8 limb planes of the centred rows x [rows, 100]."""
    out = np.zeros((x.shape[0], 3, 128), np.int64)
    out[:, :, :x.shape[1]] = digits(quantise(x, s))
    assert out.min() >= -128 and out.max() <= 127
    return out.astype(np.int8)


def fma32(a, b, c):
    """fl32(a b + c) of float32 arrays, one rounding: a b is exact in fp64; the fp64 sum is rounded once more only when it
    lands exactly on a float32 tie -- those elements are redone in rational arithmetic."""
    a, b, c = np.broadcast_arrays(a.astype(np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    s = a * b + c
    r = s.astype(np.float32)
    tie = (s.view(np.uint64) & np.uint64((1 << 29) - 1)) == np.uint64(1 << 28)
    for idx in np.argwhere(tie):
        idx = tuple(idx)
        exact = Fraction(float(a[idx])) * Fraction(float(b[idx])) + Fraction(float(c[idx]))
        cands = [np.nextafter(r[idx], np.float32(-np.inf)), r[idx], np.nextafter(r[idx], np.float32(np.inf))]
        r[idx] = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1))
    return r


def ring_model(ql, vl, qf, va):
    """The documented combine: per class w = a + b >= 1 the int64 limb products, then t = C1; t = fma(C2, 2^8, t);
    t = fma(C3, 2^16, t); t = fma(C4, 2^24, t); ring = fma(t, f, a_c) -- [Nq, clips] float32.  Also the dropped class 0."""
    q, v = ql.astype(np.int64), vl.astype(np.int64)
    C = [sum(q[:, a] @ v[:, w - a].T for a in range(3) if 0 <= w - a <= 2) for w in range(5)]
    assert all(np.abs(c).max() < 2 ** 24 for c in C)                         # v_cvt_f32_i32 is exact
    t = C[1].astype(np.float32)
    t = fma32(C[2].astype(np.float32), np.float32(256.0), t)
    t = fma32(C[3].astype(np.float32), np.float32(65536.0), t)
    t = fma32(C[4].astype(np.float32), np.float32(16777216.0), t)
    f = np.repeat(qf, 64)[:ql.shape[0], None]
    return fma32(t, f, va[None, :]), C[0]


# ---- 1. limbs ------------------------------------------------------------------------------------------------------------
def test_limb_planes_scales_and_constants(vfr):
    """Rows built so that the bank mean is exactly 0 and the bank scale exactly 2^20 (largest element XMAX 2^-20, every
    element a multiple of 2^-20): the device must reproduce chosen integers X -- the extreme with both signs, zeros, low
    digits of exactly -128 / 127 with their carries, an all-equal row -- digit for digit."""
    rs = np.random.RandomState(11)
    special = [XMAX, -XMAX, 0, 127, 128, -128, -129, 255, 256, 32639, 32640, 32767, 32768, -32768, -32896, -32897,
               65535, 65536, 127 * 65536 + 127 * 256 + 126, -(127 * 65536) - 128, 128 * 256 + 128, 8323072, 8355583, -8355584]
    r0 = np.zeros(100, np.int64)
    r0[:len(special)] = special
    r0[30:60] = rs.randint(-XMAX, XMAX + 1, 30)
    r2 = np.full(100, 4242421, np.int64)
    r4 = rs.randint(-200000, 200001, 100)
    Xv = np.stack([r0, -r0, r2, -r2, r4, -r4, np.zeros(100, np.int64)])
    V = (Xv * 2.0 ** -20).astype(np.float32)
    assert np.array_equal(V.astype(np.float64) * 2.0 ** 20, Xv)
    Q = np.concatenate([V[:3] * np.float32(0.37), (rs.randn(66, 100) * 1.7).astype(np.float32), np.zeros((1, 100), np.float32)])
    bank = bank_of(vfr, V, [1, 3, 2, 1])
    o = vfr.score_i8_debug(dev(Q), bank)
    assert np.array_equal(o["mu"][:100], np.zeros(100, np.float32))
    sv, epsv, l1v, vmax = o["bank_const"]
    assert vmax == XMAX * 2.0 ** -20 and sv == 2.0 ** 20
    vl = o["vlimbs"].astype(np.int64)
    assert np.array_equal(vl, planes(V, sv)) and not vl[:, :, 100:].any()
    assert np.array_equal(vl[:, 0, :100] + 256 * vl[:, 1, :100] + 65536 * vl[:, 2, :100], Xv)
    assert epsv == 0.0 and np.abs(V - Xv / sv).max() <= epsv                # (exactly representable here)
    assert abs(l1v - np.abs(Xv).sum(1).max() / sv) <= 1e-11 * l1v
    # queries: one scale per 64-query group, from the group's largest centred element
    for g in range(2):
        qg = Q[64 * g:64 * g + 64].astype(np.float64)
        sq = XMAX / np.abs(qg).max() if np.abs(qg).max() > 0 else 1.0
        assert o["query_scale"][g] == sq
        Xq = quantise(qg, sq)
        got = o["qlimbs"][64 * g:64 * g + 64].astype(np.int64)
        assert np.array_equal(got, planes(qg, sq)) and not got[:, :, 100:].any()
        assert np.array_equal(got[:, 0, :100] + 256 * got[:, 1, :100] + 65536 * got[:, 2, :100], Xq)
        l1, err = o["query_const"][64 * g:64 * g + 64].T
        assert np.all(np.abs(qg - Xq / sq).max(1) <= err) and np.all(err <= 0.5000001 / sq)
        assert np.allclose(l1, np.abs(qg).sum(1), rtol=1e-12, atol=0)
        assert o["query_factor"][g] == np.float32(-512.0 / (sq * sv))
    assert np.abs(o["qlimbs"][:64]).max() >= 127                            # the group's extreme element uses the whole range


# ---- 2. integer product and bound ------------------------------------------------------------------------------------
def _rows(kind, rs, n):
    x = rs.randn(n, 100) * 0.3
    if kind == "offset":
        x += 40 * 0.3 * np.random.RandomState(99).randn(1, 100)              # a common offset of 40 times the spread
    return x.astype(np.float32)


@pytest.mark.parametrize("kind", ["gauss", "offset", "outlier"])
def test_integer_product_combine_and_bound(vfr, kind):
    """70 queries (a full group and one of 6 with inactive lanes) x videos of 1, 21, 5, 16, 17 clips (60 clips: tiles span video
    boundaries, the last is partial): the device's ring values d~^2 - b_q equal the numpy model of the limb products and the
    documented combine bit for bit, and |d~^2 - d*^2| <= E2 against the fp64 distance of the ORIGINAL rows."""
    rs = np.random.RandomState({"gauss": 1, "offset": 2, "outlier": 3}[kind])
    V, Q = _rows(kind, rs, 60), _rows(kind, rs, 70)
    if kind == "outlier":
        V[37, 61] = 300.0                                                   # one centred element 10^3 times the rest
    eps = 1e-6
    bank = bank_of(vfr, V, [1, 21, 5, 16, 17])
    o = vfr.score_i8_debug(dev(Q), bank, eps)
    mu = o["mu"][:100]
    sv = o["bank_const"][0]
    vc, qc = V - mu, Q - mu                                                  # fp32, as the pre-passes centre
    assert sv == XMAX / float(np.abs(vc).max())
    assert np.array_equal(o["vlimbs"], planes(vc, sv))
    ql = np.concatenate([planes(qc[64 * g:64 * g + 64], o["query_scale"][g]) for g in range(2)])
    assert np.array_equal(o["qlimbs"], ql)
    ring, C0 = ring_model(o["qlimbs"], o["vlimbs"], o["query_factor"], o["va"])
    assert np.array_equal(o["ring"].view(np.uint32), ring.view(np.uint32)), "ring values differ from the numpy model of the combine"
    # the dropped class stays inside its term of the bound
    W = 1.0 / (np.repeat(o["query_scale"], 64)[:70, None] * sv)
    assert np.all(2 * np.abs(C0) * W <= 2 * 100 * 2 ** 14 * W)
    # the margin, on the original rows
    d2_star = ((V.astype(np.float64)[None] - Q.astype(np.float64)[:, None] + eps) ** 2).sum(-1)
    d2_approx = (o["ring"] + o["qmeta"][:, 0:1]).astype(np.float64)         # the kernel's fp32 add of b_q
    E2 = o["qmeta"][:, 2:3].astype(np.float64)
    ratio = np.abs(d2_approx - d2_star) / E2
    G = (np.sqrt((vc.astype(np.float64) ** 2).sum(1)).max() + np.sqrt((qc.astype(np.float64) ** 2).sum(1))) ** 2
    print(f"[{kind}] max |d~2 - d*2| / E2 = {ratio.max():.3f}; E2 = {(E2[:, 0] / (U * G)).min():.2f} .. {(E2[:, 0] / (U * G)).max():.2f} u G")
    assert np.all(ratio <= 1.0), ratio.max()


# ---- 3. self-check ---------------------------------------------------------------------------------------------------------
def test_int8_selfcheck_passes_and_can_fail(vfr):
    assert vfr.mfma_selfcheck_i8(DEV) == 0
    assert vfr.mfma_selfcheck_i8(DEV, permuted_reference=True) > 0
    assert vfr._mfma_mode_ok(torch.device(DEV)) and vfr.get_option("score_i8") in (0, 1)


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------
def _case(name):
    rs = np.random.RandomState(sum(map(ord, name)))
    if name == "1x1x1":
        nq, counts, k = 1, [1], 1
    elif name == "ragged":
        nq, counts, k = 5, [1, 21, 7], 10
    elif name == "65x40x21":
        nq, counts, k = 65, [21] * 40, 100
    elif name == "130x300x6":
        nq, counts, k = 130, [6] * 300, 7
    elif name == "k_above_moments":
        nq, counts, k = 9, [2, 1, 3], 40                                     # 10 moments
    elif name == "planted":
        nq, counts, k = 130, list(rs.randint(3, 22, 200)), 50
    elif name == "copies":
        nq, counts, k = 70, [21] * 30, 2                                     # k + MF_EXTRA = 30: the k'-th candidate is a copy of the k-th
    elif name == "outlier":
        nq, counts, k = 70, list(rs.randint(1, 22, 150)), 20
    V = (rs.randn(int(np.sum(counts)), 100) * 0.2).astype(np.float32)
    Q = (rs.randn(nq, 100) * 0.2).astype(np.float32)
    if name == "planted":                                                    # every query next to some clip: keys in the near tail, wide windows
        Q = (V[rs.randint(0, len(V), nq)] + rs.randn(nq, 100) * 0.02).astype(np.float32)
    if name == "copies":
        V = np.tile(V[:21], (30, 1))
    if name == "outlier":
        V[len(V) // 2, 17] = 200.0
    return Q, V, counts, k


def _score_three_ways(vfr, Q, bank, k, label):
    """`score_i8` 1 and 0 and the exact kernels, with two rank keys taken from the exact top-k: everything identical."""
    nq = Q.shape[0]
    dx, ix, _ = vfr.score_topk(Q, bank, k, mode="exact")
    kk = int((ix[0] >= 0).sum())
    p0, p1 = min(3, kk - 1), kk - 1
    rd = torch.stack([dx[:, p0], dx[:, p1]]).contiguous()
    ri = torch.stack([ix[:, p0], ix[:, p1]]).contiguous()
    _, _, cx = vfr.score_topk(Q, bank, k, rd, ri, mode="exact")
    assert cx.tolist() == [[p0] * nq, [p1] * nq]                          # (ties broken by moment id: the count is the position)
    stats = {}
    for i8 in (1, 0):
        vfr.set_option("score_i8", i8)
        ws = vfr.topk_workspace(nq, bank.num_videos, k, DEV, total_clips=bank.total_clips)
        d, i, c = vfr.score_topk(Q, bank, k, rd, ri, workspace=ws, mode="mfma")
        stats[i8] = vfr.score_mfma_stats(ws, nq, bank, k)
        assert torch.equal(i, ix) and torch.equal(d, dx) and torch.equal(c, cx), (label, i8)
        d, i, c = vfr.score_topk(Q, bank, 0, rd, ri, workspace=ws, mode="mfma")       # rank counts alone, bank products reused
        assert torch.equal(c, cx), (label, i8, "k = 0")
    print(f"[{label}] re-scored pairs: int8 {stats[1]['exact_pair_fraction']:.4f} (fallback groups {stats[1]['fallback_groups']}), "
          f"fp32 {stats[0]['exact_pair_fraction']:.4f} (fallback groups {stats[0]['fallback_groups']})")
    return stats


@pytest.mark.parametrize("name", ["1x1x1", "ragged", "65x40x21", "130x300x6", "k_above_moments", "planted", "copies", "outlier"])
def test_end_to_end_identical(vfr, name):
    Q, V, counts, k = _case(name)
    stats = _score_three_ways(vfr, dev(Q), bank_of(vfr, V, counts), k, name)
    if name == "copies":                                                     # 30 equal scores inside any margin: handed to the exact kernels
        assert stats[1]["fallback_groups"] > 0


def test_bank_rewritten_in_place_recomputes_the_limbs(vfr):
    """Same bank tensors, same workspace, new contents: the signature guard recomputes the limb planes and the bank constants
    (a stale scale would clamp the larger rows); switching `score_i8` on a kept workspace recomputes too."""
    rs = np.random.RandomState(77)
    counts = [21] * 40
    V = (rs.randn(840, 100) * 0.2).astype(np.float32)
    V2 = (rs.randn(840, 100) * 0.9 + 0.4).astype(np.float32)
    Q = dev((rs.randn(65, 100) * 0.2).astype(np.float32))
    bank = bank_of(vfr, V, counts)
    ws = vfr.topk_workspace(65, 40, 10, DEV, total_clips=840)
    for step, i8 in enumerate((1, 1, 0, 1)):
        vfr.set_option("score_i8", i8)
        if step == 1:
            bank.emb.copy_(dev(V2))
        d, i, _ = vfr.score_topk(Q, bank, 10, workspace=ws, mode="mfma")
        dx, ix, _ = vfr.score_topk(Q, bank, 10, mode="exact")
        assert torch.equal(i, ix) and torch.equal(d, dx), step
        print(f"[rewrite step {step}] {vfr.score_mfma_stats(ws, 65, bank, 10)}")
