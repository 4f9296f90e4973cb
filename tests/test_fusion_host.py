"""Late-fusion retrieval without a GPU: the CPU provider against the numpy statement of tests/fusion_reference.py on the oracle's
dense moment scores (both levels, rank counts, own rows), the two identities against the single-stream entry points, the refusals
of fuse_corpora / evaluate_fusion, evaluate_fusion with weights (1, 0) against evaluate, a gloo world of 2 through
engine.corpus_fusion_topk, and the C entry points' host-side argument checks and workspace bound."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fusion_reference import fused_scores, level_keys, own_rows, split_keys, statement
from helpers import MemoryDataset, make_model, problem

CPU_THREADS = 1
DIMS = (100, 37, 4)
WEIGHTS = (0.5, 0.25, 2.0)


def _streams(seed, counts, S, nq=7, dims=DIMS):
    rs = np.random.RandomState(seed)
    counts = np.asarray(counts, np.int64)
    total = int(counts.sum())
    Vs = [(rs.randn(total, D) * 0.3).astype(np.float32) for D in dims[:S]]
    Qs = [(rs.randn(nq, D) * 0.3).astype(np.float32) for D in dims[:S]]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return Qs, Vs, counts, off


def _mixed_counts(nv, seed):
    c = np.random.RandomState(seed).randint(1, 22, nv).astype(np.int64)
    c[0] = c[-1] = 21
    return c


def _banks(ops, Vs, off, id_base=0):
    return [ops.make_bank(torch.from_numpy(V), torch.from_numpy(off), id_base) for V in Vs]


def _t(arrs):
    return [torch.from_numpy(a) for a in arrs]


@pytest.mark.parametrize("S", [1, 2, 3])
def test_cpu_provider_matches_reference(oracle, S):
    from vfr_amd import engine
    ops = engine.TorchCpuOps()
    Qs, Vs, counts, off = _streams(S, _mixed_counts(9, S), S)
    id_base = 11
    banks = _banks(ops, Vs, off, id_base)
    Scs = [oracle.score_moments(Q, V, off) for Q, V in zip(Qs, Vs)]
    w = WEIGHTS[:S]
    nq = Qs[0].shape[0]
    for level in ("moments", "videos"):
        K = level_keys(fused_scores(Scs, counts, w), counts, level, id_base)
        srt = np.sort(K, axis=1)
        # one rank key present in the bank, one strictly between two keys
        rk = np.stack([srt[:, min(3, srt.shape[1] - 1)], srt[:, min(5, srt.shape[1] - 1)] + np.uint64(1)])
        rd, ri = split_keys(rk)
        for k in (0, 1, 16, 448):
            d, i, c = ops.score_fusion(_t(Qs), banks, w, k, level, torch.from_numpy(rd), torch.from_numpy(ri))
            wd, wi, wc = statement(Scs, counts, w, k, level, id_base, rk)
            if k:
                assert np.array_equal(d.numpy(), wd) and np.array_equal(i.numpy(), wi), (S, level, k)
            assert np.array_equal(c.numpy(), wc), (S, level, k)
        assert wc[0].tolist() == [min(3, srt.shape[1] - 1)] * nq
    own = (np.arange(nq) * 4) % len(counts)
    got = ops.score_fusion_own(_t(Qs), banks, w, torch.from_numpy(own.astype(np.int32)))
    assert np.array_equal(got.numpy(), own_rows(Scs, counts, w, own))


def test_cpu_identities():
    """S = 1 with w = (1), and w = (1, 0, 0), are the single-stream entry points on stream 0, bit for bit."""
    from vfr_amd import engine
    ops = engine.TorchCpuOps()
    Qs, Vs, counts, off = _streams(5, _mixed_counts(8, 5), 3)
    banks = _banks(ops, Vs, off, 7)
    Q0 = torch.from_numpy(Qs[0])
    nq = Q0.shape[0]
    keys = ops._dense_keys(Q0, banks[0]).numpy().astype(np.uint64)
    rk = keys[np.arange(nq), (np.arange(nq) * 13) % keys.shape[1]][None]
    rd, ri = (torch.from_numpy(x) for x in split_keys(rk))
    for Qx, bx, w in ((_t(Qs[:1]), banks[:1], (1.0,)), (_t(Qs), banks, (1.0, 0.0, 0.0))):
        for k in (1, 10, 100):
            d, i, c = ops.score_fusion(Qx, bx, w, k, "moments", rd, ri)
            wd, wi, wc = ops.score_topk(Q0, banks[0], k, rd, ri)
            assert torch.equal(d, wd) and torch.equal(i, wi) and torch.equal(c, wc)
            d, i, c = ops.score_fusion(Qx, bx, w, k, "videos", rd, ri)
            wd, wi, wc = ops.score_video_topk(Q0, banks[0], k, rd[0], ri[0])
            assert torch.equal(d, wd) and torch.equal(i, wi) and torch.equal(c[0], wc)
        own = torch.from_numpy((np.arange(nq) % len(counts)).astype(np.int32))
        assert torch.equal(ops.score_fusion_own(Qx, bx, w, own), ops.score_own(Q0, banks[0], own))


def test_fuse_corpora_refusals():
    from vfr_amd import engine
    ops = engine.TorchCpuOps()
    Qs, Vs, counts, off = _streams(6, [3, 5, 2, 4], 2)
    a = engine.corpus_from_embeddings(torch.from_numpy(Vs[0]), counts, "cpu", ops)
    b = engine.corpus_from_embeddings(torch.from_numpy(Vs[1]), counts, "cpu", ops)
    fused = engine.fuse_corpora([a, b], (0.6, 0.4), names=[["a", "b", "c", "d"]] * 2)
    assert fused.weights.dtype == np.float32 and fused.names == ["a", "b", "c", "d"] and len(fused.banks) == 2
    other = np.asarray([3, 5, 4, 2])                                        # the same clips, cut differently
    c = engine.corpus_from_embeddings(torch.from_numpy(Vs[1]), other, "cpu", ops)
    with pytest.raises(ValueError, match="clip counts"):
        engine.fuse_corpora([a, c], (0.5, 0.5))
    half = engine.corpus_from_embeddings(torch.from_numpy(Vs[1]), counts, "cpu", ops, rank=1, world=2)
    with pytest.raises(ValueError, match="holds videos"):
        engine.fuse_corpora([a, half], (0.5, 0.5))
    with pytest.raises(ValueError, match="order"):
        engine.fuse_corpora([a, b], (0.5, 0.5), names=[["a", "b", "c", "d"], ["a", "c", "b", "d"]])
    for bad in ((0.5, -0.1), (0.5, float("nan")), (float("inf"), 1.0), (1.0,), (1.0, 1.0, 1.0)):
        with pytest.raises(ValueError):
            engine.fuse_corpora([a, b], bad)
    with pytest.raises(ValueError):
        engine.fuse_corpora([a] * 5, (1.0,) * 5)
    # the provider refuses banks that do not describe the same videos
    with pytest.raises(ValueError):
        ops.score_fusion(_t(Qs), [a.bank, c.bank], (0.5, 0.5), 3)
    with pytest.raises(ValueError):
        engine.corpus_fusion_topk(fused, _t(Qs)[:1], 3, ops=ops)


def _dataset(p):
    return MemoryDataset(p["seg"], p["ctx"], p["counts"], p["tokens"], p["own"], p["times"])


def test_evaluate_fusion_refusals_and_identity_cpu():
    from vfr_amd import evaluate as vevaluate
    threads = torch.get_num_threads()
    torch.set_num_threads(CPU_THREADS)
    try:
        p = problem(23, 17, "didemo", feat_dim=64, hidden=16)
        ds = _dataset(p)
        model = make_model(p["sd"], feat_dim=64, hidden=16)

        def run(weights, level="moments", datasets=(ds, ds), **kw):
            its = [d.iterators() for d in datasets]
            return vevaluate.evaluate_fusion([model] * len(its), [i[0] for i in its], [i[1] for i in its], ds.annotations, "cpu", weights,
                                             level=level, **kw)
        # two copies of one model, weights (1, 0): exactly evaluate's dict (and evaluate_videos'), and its top-k
        vi, li = ds.iterators()
        want, (wd, wi) = vevaluate.evaluate(model, vi, li, ds.annotations, "cpu", return_topk=10)
        got, (d, i, v) = run((1.0, 0.0), return_topk=10)
        assert got == want and torch.equal(d, wd) and torch.equal(i, wi)
        vi, li = ds.iterators()
        assert run((1.0, 0.0), "videos") == vevaluate.evaluate_videos(model, vi, li, ds.annotations, "cpu")
        # a real fusion of a stream with itself: d + d scaled by (0.5, 0.5) is d again, bit for bit
        assert run((0.5, 0.5)) == want
        # refusals
        for bad in ((1.0, -1.0), (float("nan"), 1.0), (1.0,)):
            with pytest.raises(ValueError):
                run(bad)
        with pytest.raises(ValueError):
            run((1.0, 0.0), level="clips")
        # the same clips cut differently: two videos of different length swap their clip counts
        counts2 = p["counts"].copy()
        a = 0
        b = next(v for v in range(len(counts2)) if counts2[v] != counts2[a])
        counts2[[a, b]] = counts2[[b, a]]
        ds2 = MemoryDataset(p["seg"], p["ctx"], counts2, p["tokens"], p["own"], p["times"])
        with pytest.raises(ValueError, match="clip counts"):
            run((0.5, 0.5), datasets=(ds, ds2))
        # another video order
        ds3 = _dataset(p)
        ds3.videos = list(reversed(ds3.videos))
        with pytest.raises(ValueError):
            run((0.5, 0.5), datasets=(ds, ds3))
    finally:
        torch.set_num_threads(threads)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _sharded_case():
    Qs, Vs, counts, off = _streams(21, _mixed_counts(13, 21), 2, nq=9)
    rs = np.random.RandomState(22)
    own = rs.randint(0, len(counts), 9)
    Mmax = int(counts[own].max() * (counts[own].max() + 1) // 2)
    labels = np.zeros((2, 9, Mmax), bool)
    for q in range(9):
        M = int(counts[own[q]] * (counts[own[q]] + 1) // 2)
        labels[0, q, rs.randint(0, M, 3)] = True
        labels[1, q, rs.randint(0, M)] = True
    return Qs, Vs, counts, own, labels


def _fusion_pass(rank, world):
    from vfr_amd import engine
    ops = engine.TorchCpuOps()
    Qs, Vs, counts, own, labels = _sharded_case()
    shards = [engine.corpus_from_embeddings(torch.from_numpy(V), counts, "cpu", ops, rank, world) for V in Vs]
    fused = engine.fuse_corpora(shards, (0.6, 0.4))
    res = {}
    for level in ("moments", "videos"):
        d, i, v, r = engine.corpus_fusion_topk(fused, _t(Qs), 20, level, own_global=own, labels=torch.from_numpy(labels), ops=ops, world=world)
        res[level] = (d.numpy(), i.numpy(), v.numpy(), r.numpy())
    return res


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(CPU_THREADS)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        res = _fusion_pass(rank, world)
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), **{f"{lv}_{n}": x for lv, t in res.items() for n, x in zip("divr", t)})
    finally:
        dist.destroy_process_group()


def test_two_rank_fusion_equals_single_process(oracle, tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    threads = torch.get_num_threads()
    torch.set_num_threads(CPU_THREADS)
    try:
        ref = _fusion_pass(0, 1)
    finally:
        torch.set_num_threads(threads)
    # the one-rank pass itself is the statement: lists, and ranks = keys before the best positive key of the own video
    Qs, Vs, counts, own, labels = _sharded_case()
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    Scs = [oracle.score_moments(Q, V, off) for Q, V in zip(Qs, Vs)]
    wd, wi, _ = statement(Scs, counts, (0.6, 0.4), 20, "moments")
    assert np.array_equal(ref["moments"][0], wd) and np.array_equal(ref["moments"][1], wi)
    K = level_keys(fused_scores(Scs, counts, (0.6, 0.4)), counts, "moments")
    mo = np.concatenate([[0], np.cumsum(counts * (counts + 1) // 2)])
    for r in range(2):
        for q in range(len(own)):
            pos = mo[own[q]] + np.nonzero(labels[r, q])[0]
            assert ref["moments"][3][r, q] == int((K[q] < K[q, pos].min()).sum())
    for rk in range(2):
        got = np.load(tmp_path / f"r{rk}.npz")
        for level, t in ref.items():
            for n, x in zip("divr", t):
                assert np.array_equal(got[f"{level}_{n}"], x), (rk, level, n)


def test_capi_rejects_bad_host_arguments_without_a_gpu():
    from vfr_amd import _vfr
    lib = _vfr.lib()
    ws = ctypes.create_string_buffer(1 << 16)
    dummy = ctypes.cast(ws, ctypes.c_void_p).value      # never dereferenced: every call below fails its host-side checks

    def arrays(S, D=(100, 37, 4, 100, 8), w=(0.5, 0.25, 0.125, 2.0, 1.0), q=None, v=None):
        n = max(S, 1)
        return ((ctypes.c_void_p * n)(*([dummy] * n if q is None else q)), (ctypes.c_void_p * n)(*([dummy] * n if v is None else v)),
                (ctypes.c_int * n)(*D[:n]), (ctypes.c_float * n)(*w[:n]))

    def call(S=2, hosts=None, k=10, level=0, max_clips=21, num_rank=0, nbytes=1 << 16, wsp=dummy):
        Qh, Vh, Dh, wh = hosts if hosts is not None else arrays(S)
        return lib.vfr_score_fusion_f32(Qh, Vh, Dh, wh, S, 4, dummy, dummy, 10, 210, 21, max_clips, 1e-6, 0, level, k, dummy, dummy,
                                        num_rank, None, None, None, wsp, nbytes, None)

    def own(S=2, hosts=None, max_clips=21, Mmax=231):
        Qh, Vh, Dh, wh = hosts if hosts is not None else arrays(S)
        return lib.vfr_score_fusion_own_f32(Qh, Vh, Dh, wh, S, 4, dummy, dummy, 10, max_clips, 1e-6, Mmax, dummy, None)

    for fn in (call, own):
        assert fn(S=0) == -1 and b"S = 0" in lib.vfr_last_error()
        assert fn(S=5, hosts=arrays(5)) == -1 and b"S = 5" in lib.vfr_last_error()
        assert fn(hosts=arrays(2, w=(0.5, -0.25))) == -1 and b"weight" in lib.vfr_last_error()
        assert fn(hosts=arrays(2, w=(float("nan"), 1.0))) == -1 and fn(hosts=arrays(2, w=(1.0, float("inf")))) == -1
        assert fn(hosts=arrays(2, D=(100, 0))) == -1 and b"D = 0" in lib.vfr_last_error()
        assert fn(hosts=arrays(2, q=[dummy, None])) == -1 and b"Q is null" in lib.vfr_last_error()
        assert fn(hosts=arrays(2, v=[None, dummy])) == -1 and b"V is null" in lib.vfr_last_error()
        Qh, Vh, Dh, wh = arrays(2)
        assert fn(hosts=(None, Vh, Dh, wh)) == -1 and fn(hosts=(Qh, Vh, None, wh)) == -1 and fn(hosts=(Qh, Vh, Dh, None)) == -1
        assert b"null stream array" in lib.vfr_last_error()
        assert fn(max_clips=65) == -1
        # the LDS plan: the streams' query rows (each rounded up to 4 floats) hold at most VFR_FUSION_MAX_SUM_D = 8192 floats
        assert fn(hosts=arrays(2, D=(8192, 1))) == -2 and b"VFR_FUSION_MAX_SUM_D" in lib.vfr_last_error()
    assert call(k=449) == -1 and call(level=2) == -1 and call(num_rank=5) == -1 and call(num_rank=1) == -1
    assert b"vfr_score_fusion_f32" in lib.vfr_last_error()
    assert call(wsp=None) == -4 and call(nbytes=16) == -4                      # VFR_EWORKSPACE
    assert own(Mmax=230) == -1
    assert lib.vfr_version() == 100


def test_workspace_is_bounded_by_the_chunk_plan():
    from vfr_amd import _vfr
    lib = _vfr.lib()
    wsb = lib.vfr_score_fusion_workspace_bytes
    # the benchmark shape: 5 000 queries run whole-bank streams (one chunk): Nq x k keys, whatever Nv is
    assert wsb(5000, 10000, 100) == 5000 * 100 * 8 + 256
    assert wsb(5000, 10_000_000, 100) == wsb(5000, 10000, 100)
    # one query: one chunk per block of 64 videos up to the bound of 256 chunks, then no growth with Nv
    assert wsb(1, 64 * 128, 100) == 128 * 100 * 8 + 256
    assert wsb(1, 64 * 256, 100) == wsb(1, 1 << 30, 100) == 256 * 100 * 8 + 256
    assert wsb(1, 0, 16) > 0 and wsb(0, 100, 16) > 0
    assert wsb(5000, 10000, 449) == 0 and wsb(-1, 10, 1) == 0 and wsb(1 << 31, 10, 1) == 0
