"""Windowed retrieval on the GPU (vfr_score_window_f32, vfr_score_window_span_keys_f32, engine.corpus_window_topk,
evaluate.evaluate_windowed) against the numpy statement of tests/window_reference.py on the oracle's dense moment scores, bit for bit
in distances, ids and counts; the identities against the device's own score_topk and score_prior."""
import numpy as np
import pytest
import torch

from fusion_reference import moment_offsets, split_keys
from helpers import MemoryDataset, make_model
from window_reference import KEY_EMPTY, rank_keys, span_keys, statement

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENGTHS = (1, 2, 7, 64)
KS = (0, 1, 100, 448)
ID_BASE = 9
# several videos inside one tile of 64 flat clips, videos across tiles, an empty video, a last tile shorter than 64, and two pairs of
# identical videos (0, 10) and (6, 11): exact ties across videos, decided by id
MIXED = [5, 0, 1, 63, 64, 65, 2, 129, 300, 7, 5, 2]
SAME = ((0, 10), (6, 11))


@pytest.fixture(scope="module")
def vfr():
    from vfr_amd import _vfr
    _vfr.lib()
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return _vfr


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype else t).to(DEV)


def case(counts, D=100, seed=0, nq=3, same=()):
    rs = np.random.RandomState(seed)
    counts = np.asarray(counts, np.int64)
    off = np.concatenate([[0], np.cumsum(counts)])
    V = (rs.randn(int(off[-1]), D) * 0.3).astype(np.float32)
    for a, b in same:
        assert counts[a] == counts[b]
        V[off[b]:off[b + 1]] = V[off[a]:off[a + 1]]
    Q = (rs.randn(nq, D) * 0.3).astype(np.float32)
    return Q, V, counts, off.astype(np.int32)


def queries(Q, odd=False):
    """The query matrix on the device; ``odd``: a view that starts one float into its storage (rows not 16-byte aligned)."""
    if not odd:
        return dev(Q)
    store = torch.zeros(Q.size + 1, dtype=torch.float32, device=DEV)
    store[1:] = dev(Q).reshape(-1)
    view = store[1:].view(Q.shape)
    assert view.storage_offset() == 1 and view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def plan_chunks(nq, total_clips, target=4096, max_chunks=256):
    """scan_plan of csrc/scan_common.h: the chunks the flat clip axis is cut into."""
    blocks = -(-total_clips // 64)
    want = min(-(-target // max(nq, 1)), max_chunks)
    c = max(1, min(want, blocks))
    per = -(-max(blocks, 1) // c) * 64
    return -(-max(total_clips, 1) // per), c, per


def run(vfr, Qd, bank, L, k, rk=None, count_lt=None):
    rd = ri = None
    if rk is not None:
        rd, ri = (dev(x) for x in split_keys(rk))
    d, i, c = vfr.score_window(Qd, bank, L, k, rd, ri, count_lt=count_lt)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (d, i, c))


def check(vfr, Sc, Q, V, counts, off, lengths=LENGTHS, ks=KS, odd=False, what=""):
    bank = vfr.VideoBank(dev(V), dev(off), ID_BASE)
    Qd = queries(Q, odd)
    for L in lengths:
        rk = rank_keys(Sc, counts, L, ID_BASE)                                    # first, middle, last and one absent key
        for k in ks:
            d, i, c = run(vfr, Qd, bank, L, k, rk)
            wd, wi, wc = statement(Sc, counts, L, k, ID_BASE, rk)
            if k:
                assert np.array_equal(i, wi), f"{what}: ids differ (L = {L}, k = {k})"
                assert np.array_equal(d, wd), f"{what}: distances differ (L = {L}, k = {k})"
            else:
                assert d is None and i is None
            assert np.array_equal(c, wc), f"{what}: counts differ (L = {L}, k = {k})"
        before = torch.full((4, len(Q)), 5, dtype=torch.int64, device=DEV)
        _, _, c = run(vfr, Qd, bank, L, ks[-1], rk, count_lt=before)
        assert np.array_equal(c, statement(Sc, counts, L, 0, ID_BASE, rk)[2] + 5), f"{what}: added counts differ (L = {L})"


@pytest.mark.parametrize("D,odd", [(100, False), (36, True)])
@pytest.mark.parametrize("nq", [3, 70])
def test_mixed_bank(vfr, oracle, nq, D, odd):
    """643 flat clips at Nq = 3 and Nq = 70: the axis is cut into several chunks that ignore video boundaries -- the 129- and the
    300-clip video straddle chunk boundaries -- in both code forms."""
    Q, V, counts, off = case(MIXED, D, seed=nq + D, nq=nq, same=SAME)
    chunks, bound, _ = plan_chunks(nq, int(off[-1]))
    assert chunks > 1
    assert vfr.lib().vfr_score_window_workspace_bytes(nq, int(off[-1]), 100) == (bound * nq * 100 * 8 + 256 + 255) // 256 * 256
    Sc = oracle.score_moments(Q, V, off)
    mo = moment_offsets(counts)
    for a, b in SAME:
        assert np.array_equal(Sc[:, mo[a]:mo[a + 1]], Sc[:, mo[b]:mo[b + 1]])
    check(vfr, Sc, Q, V, counts, off, odd=odd, what=f"Nq = {nq}, D = {D}")


@pytest.mark.parametrize("D,odd", [(100, False), (36, True)])
@pytest.mark.parametrize("nq", [2100, 4200])
def test_many_tiles_per_chunk(vfr, oracle, nq, D, odd):
    """Enough queries that a wave walks several tiles of the 643-clip axis: Nq = 2 100 gives two chunks of 384 and 259 clips (six and
    five tiles, the last one short), Nq = 4 200 one chunk of all eleven tiles.  The tile loop carries the list, its threshold and the
    rank counters from tile to tile, overwrites the distances of the previous tile, and meets each halo again as the next tile's body.
    The queries are seven distinct rows repeated (a wave does not know), so the reference is computed for seven."""
    Q7, V, counts, off = case(MIXED, D, seed=nq + D, nq=7, same=SAME)
    chunks, bound, per = plan_chunks(nq, int(off[-1]))
    assert per >= 128 and (chunks > 1 if nq == 2100 else chunks == 1)
    assert vfr.lib().vfr_score_window_workspace_bytes(nq, int(off[-1]), 100) == (bound * nq * 100 * 8 + 256 + 255) // 256 * 256
    Sc = oracle.score_moments(Q7, V, off)
    rep = np.arange(nq) % 7
    bank = vfr.VideoBank(dev(V), dev(off), ID_BASE)
    Qd = queries(np.ascontiguousarray(Q7[rep]), odd)
    for L in LENGTHS:
        rk7 = rank_keys(Sc, counts, L, ID_BASE)
        rk = np.ascontiguousarray(rk7[:, rep])
        wc = statement(Sc, counts, L, 0, ID_BASE, rk7)[2][:, rep]
        for k in KS:
            d, i, c = run(vfr, Qd, bank, L, k, rk)
            if k:
                wd, wi, _ = statement(Sc, counts, L, k, ID_BASE)
                assert np.array_equal(i, wi[rep]), f"ids differ (L = {L}, k = {k})"
                assert np.array_equal(d, wd[rep]), f"distances differ (L = {L}, k = {k})"
            assert np.array_equal(c, wc), f"counts differ (L = {L}, k = {k})"
        before = torch.full((4, nq), 5, dtype=torch.int64, device=DEV)
        _, _, c = run(vfr, Qd, bank, L, KS[-1], rk, count_lt=before)
        assert np.array_equal(c, wc + 5), f"added counts differ (L = {L})"


@pytest.mark.parametrize("D,odd", [(100, False), (36, True)])
def test_one_chunk(vfr, oracle, D, odd):
    """A bank of 43 clips is one chunk and one short tile whatever Nq is."""
    Q, V, counts, off = case([5, 0, 1, 30, 7], D, seed=D, nq=70)
    assert plan_chunks(70, int(off[-1]))[0] == 1
    check(vfr, oracle.score_moments(Q, V, off), Q, V, counts, off, odd=odd, what=f"one chunk, D = {D}")


@pytest.mark.parametrize("D,odd", [(100, False), (36, True)])
def test_a_1024_clip_video(vfr, oracle, D, odd):
    """One 1 024-clip video between two short ones: 17 tiles, the video crosses every chunk boundary."""
    Q, V, counts, off = case([3, 1024, 6], D, seed=1024 + D, nq=3)
    assert plan_chunks(3, int(off[-1]))[0] > 1
    check(vfr, oracle.score_moments(Q, V, off), Q, V, counts, off, odd=odd, what=f"1024 clips, D = {D}")


def test_identity_with_the_existing_device_paths(vfr):
    """Counts in 1 .. 21: L = 64 is score_topk (exact kernels), L = 5 is score_prior under moment_table(21, max_len=5)."""
    from vfr_amd import engine
    counts = np.random.RandomState(4).randint(1, 22, 90)
    counts[[0, -1]] = 21
    Q, V, counts, off = case(counts, seed=4, nq=11)
    bank = vfr.VideoBank(dev(V), dev(off), ID_BASE)
    Qd = dev(Q)
    table = engine.moment_table(21, max_len=5).on(DEV)
    for k in (1, 100, 448):
        wd, wi, _ = vfr.score_topk(Qd, bank, k, mode="exact")
        rd, ri = wd[:, k // 2].contiguous(), wi[:, k // 2].contiguous()
        wd, wi, wc = vfr.score_topk(Qd, bank, k, rd, ri, mode="exact")
        d, i, c = vfr.score_window(Qd, bank, 64, k, rd, ri)
        torch.cuda.synchronize()
        assert torch.equal(d, wd) and torch.equal(i, wi) and torch.equal(c, wc), k
        wd, wi, wc = vfr.score_prior(Qd, bank, table, k, "moments", rd, ri)
        d, i, c = vfr.score_window(Qd, bank, 5, k, rd, ri)
        torch.cuda.synchronize()
        assert torch.equal(d, wd) and torch.equal(i, wi) and torch.equal(c, wc), k


def test_span_keys(vfr, oracle):
    """Three shards of the mixed bank, each with its vid_base and id_base: repeated and unsorted items, spans of 1 and 64 clips inside
    the 300-clip video, items of other shards left untouched; MIN over the shards gives every key."""
    Q, V, counts, off = case(MIXED, seed=21, nq=5)
    Sc = oracle.score_moments(Q, V, off)
    mo = moment_offsets(counts)
    bank = vfr.VideoBank(dev(V), dev(off), ID_BASE)
    Qd = dev(Q)
    items = np.asarray([(4, 8, 236, 299), (0, 8, 17, 17), (1, 3, 0, 62), (1, 7, 60, 123), (0, 8, 17, 17), (2, 11, 0, 1), (3, 0, 4, 4),
                        (4, 8, 0, 63), (2, 5, 1, 64), (0, 2, 0, 0), (3, 9, 2, 6)], np.int32)
    whole, bad = span_keys(Sc, counts, items, ID_BASE)
    assert bad == 0 and (whole != KEY_EMPTY).all()
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = vfr.window_span_keys(Qd, bank, dev(items), bad=flag)
    assert np.array_equal(got.cpu().numpy().view(np.uint64), whole) and int(flag.item()) == 0
    red = torch.full((len(items),), 0x7F800000FFFFFFFF, dtype=torch.int64, device=DEV)
    for a, z in ((0, 4), (4, 8), (8, 12)):
        sub = vfr.slice_bank(bank, counts, a, z)
        got = vfr.window_span_keys(Qd, sub, dev(items), vid_base=a, bad=flag)
        want, _ = span_keys(Sc[:, mo[a]:mo[z]], counts[a:z], items, ID_BASE + int(mo[a]), vid_base=a)
        assert np.array_equal(got.cpu().numpy().view(np.uint64), want), (a, z)
        assert (want != KEY_EMPTY).any() and (want == KEY_EMPTY).any()
        red = torch.minimum(red, got)
    assert np.array_equal(red.cpu().numpy().view(np.uint64), whole) and int(flag.item()) == 0
    # the generic width on a query view with an odd storage offset
    Q36, V36, _, _ = case(MIXED, 36, seed=22, nq=5)
    got = vfr.window_span_keys(queries(Q36, odd=True), vfr.VideoBank(dev(V36), dev(off), ID_BASE), dev(items))
    assert np.array_equal(got.cpu().numpy().view(np.uint64), span_keys(oracle.score_moments(Q36, V36, off), counts, items, ID_BASE)[0])
    # malformed items: the flag, the slot untouched, the neighbours what they were
    for wrong in [(5, 8, 0, 1), (-1, 8, 0, 1), (0, 8, -1, 1), (0, 8, 4, 3), (0, 8, 0, 300), (0, 8, 0, 64), (0, 1, 0, 0), (0, 3, 62, 63)]:
        mixed = np.concatenate([items[:3], np.asarray([wrong], np.int32), items[3:6]])
        out = torch.full((len(mixed),), 12345, dtype=torch.int64, device=DEV)
        flag.zero_()
        vfr.window_span_keys(Qd, bank, dev(mixed), out=out, bad=flag)
        want, bad = span_keys(Sc, counts, mixed, ID_BASE)
        assert bad == 1 and int(flag.item()) == 1 and int(out[3]) == 12345, wrong
        assert np.array_equal(np.delete(out.cpu().numpy().view(np.uint64), 3), np.delete(want, 3)), wrong
    empty = vfr.window_span_keys(Qd, bank, torch.zeros((0, 4), dtype=torch.int32, device=DEV))
    assert empty.shape == (0,)


def test_argument_refusal(vfr):
    """VFR_EINVAL before anything is enqueued, the reason in vfr_last_error()."""
    lib = vfr.lib()
    Q, V, counts, off = case([4, 3], seed=1, nq=2)
    bank = vfr.VideoBank(dev(V), dev(off), 0)
    Qd = dev(Q)
    od, oi = torch.full((2, 449), 7.0, device=DEV), torch.full((2, 449), 7, dtype=torch.int64, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)

    def call(q=Qd.data_ptr(), nq=2, max_clips=4, max_len=3, k=4, ws_bytes=ws.numel()):
        return lib.vfr_score_window_f32(q, nq, bank.emb.data_ptr(), bank.clip_off.data_ptr(), bank.mom_off.data_ptr(), 2, 7, max_clips,
                                        100, 1e-6, 0, max_len, k, od.data_ptr(), oi.data_ptr(), 0, 0, 0, 0, ws.data_ptr(), ws_bytes, 0)
    for kw, word in ((dict(max_len=0), b"max_len"), (dict(max_len=65), b"max_len"), (dict(max_clips=1025), b"max_clips"),
                     (dict(k=449), b"k <= 448"), (dict(ws_bytes=8), b"workspace"), (dict(q=0), b"Q is null")):
        assert call(**kw) == -1, kw
        assert word in lib.vfr_last_error(), (kw, lib.vfr_last_error())
    assert lib.vfr_score_window_workspace_bytes(2, 7, 449) == 0
    torch.cuda.synchronize()
    assert bool((od == 7.0).all()) and bool((oi == 7).all())                       # nothing was launched
    assert call() == 0
    with pytest.raises(RuntimeError, match="ROCm device"):
        vfr.score_window(torch.from_numpy(Q), bank, 3, 4)
    with pytest.raises(RuntimeError, match="float32"):
        vfr.score_window(Qd.double(), bank, 3, 4)


def test_empty_shapes(vfr):
    """Nq = 0: nothing to write; a bank without videos or clips: padding and untouched counts; videos without clips own nothing."""
    Q, V, counts, off = case([3, 1, 2, 4], seed=1, nq=0)
    bank = vfr.VideoBank(dev(V), dev(off), 0)
    d, i, c = run(vfr, dev(Q), bank, 4, 16)
    assert d.shape == (0, 16) and i.shape == (0, 16) and c is None
    none = vfr.VideoBank(torch.zeros((0, 100), dtype=torch.float32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV), 4)
    hollow = vfr.VideoBank(torch.zeros((0, 100), dtype=torch.float32, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV), 4)
    Q11 = np.random.RandomState(1).randn(11, 100).astype(np.float32)
    rk = np.stack([np.full(11, (0x3F800000 << 32) | 7, np.uint64)] * 2)
    for b in (none, hollow):
        before = torch.full((2, 11), 3, dtype=torch.int64, device=DEV)
        d, i, c = run(vfr, dev(Q11), b, 4, 16, rk, count_lt=before)
        assert np.all(np.isinf(d)) and np.all(i == -1) and np.all(c == 3)
        _, _, c = run(vfr, dev(Q11), b, 4, 0, rk, count_lt=before)
        assert np.all(c == 3)


def test_evaluate_windowed_gpu_equals_cpu():
    """A 12-video problem with one 150-clip video: the metric dicts and the unreachable shares of cuda:0 equal the CPU device's."""
    from vfr_amd import evaluate as vevaluate
    from vfr_amd import synth
    counts = synth.clip_counts(12, "didemo", seed=31)
    counts[4] = 150
    seg, ctx = synth.video_features(counts, 64, seed=31)
    tokens = synth.query_tokens(16, vocab=400, seed=31)
    own, times = synth.annotations(16, counts, seed=31)
    own[:3] = 4                                                                    # three queries on the long video
    rs = np.random.RandomState(31)
    for q in range(3):
        s = int(rs.randint(0, 120))
        times[q] = [[s, s + 9], [s + 1, s + 10], [s + 40, s + 41], [s, s + 9]]
    sd = synth.model_weights(64, vocab=400, hidden=16, seed=31)
    res = {}
    for device in ("cpu", DEV):
        for L in (4, 16):
            ds = MemoryDataset(seg, ctx, counts, tokens, own, times)
            model = make_model(sd, feat_dim=64, hidden=16).to(device)
            res[(device, L)] = vevaluate.evaluate_windowed(model, *ds.iterators(), ds.annotations, device, L)
    for L in (4, 16):
        assert res[("cpu", L)] == res[(DEV, L)], L
    assert res[(DEV, 4)]["unreachable"]["IoU=0.5"] > 0 and res[(DEV, 16)]["unreachable"]["IoU=0.5"] == 0
