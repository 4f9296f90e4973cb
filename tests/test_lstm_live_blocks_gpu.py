"""Fused LSTM step, option `lstm_live_blocks`: a wave issues fragment reads, MFMAs, the table gather and the gate epilogue only
for its 16-row blocks that hold a row below the direction's active count and a unit below H.  The result must be the SAME
BITS as with every block issued (`lstm_live_blocks` 0) and as the CPU oracle, and a debug counter in the workspace must show
that exactly the live blocks were issued.

Shapes: E = 100, D = 100, T = 5.  H = 104 is four column tiles of 32 units, the last with 8 real units: its second 16-unit half
is dead (H % 32 = 8 keeps the select-free instantiation eligible, as at H = 1000); H = 96 is the control without a dead half.
B + 1 rows (row 0 is the all-pad row) end a 64-row tile with 1, 2, 3 and 4 live 16-row blocks (B = 72 -> 73 rows = 64 + 9, the
bench's 9-row last tile; 80, 96, 112), a 128-row and a 32-row tile mid-block (127 -> 128 rows is the full control, 200 -> 201
rows = 128 + 73 = 6 x 32 + 9); every batch runs with the tile height chosen by size and forced to 64, 128 and 32 rows.  The
token lengths cover 0 .. T, so the reverse direction's active prefix ends in a different block at every step."""
import numpy as np
import pytest
import torch

from helpers import lstm_of
from vfr_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E, T, VOCAB = 100, 5, 400
HS, BS, TILES = (104, 96), (72, 80, 96, 112, 127, 200), (0, 1, 2, 3)
TILE_ROWS = {1: 64, 2: 128, 3: 32}


@pytest.fixture(scope="module")
def vfr():
    from vfr_amd import _vfr
    _vfr.lib()
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return _vfr


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def make_tokens(B, seed):
    """Every length 0 .. T occurs (an all-pad query and a full-length one among them), in shuffled order."""
    rs = np.random.RandomState(seed)
    lens = rs.permutation(np.arange(B) % (T + 1))
    tok = np.zeros((B, T), np.int64)
    for i, n in enumerate(lens):
        tok[i, :n] = rs.randint(1, VOCAB, size=n)
    assert set(lens.tolist()) == set(range(T + 1))
    return tok, lens


_CASES = {}


def case(H, B, oracle, rows=None):
    """Inputs of one (H, B) and their oracle embeddings (of the queries `rows`; all by default): computed once, shared by the
    tests, never modified."""
    if (H, B) not in _CASES:
        sd = synth.model_weights(64, vocab=VOCAB, hidden=H, seed=100 + H)
        tok, lens = make_tokens(B, seed=B)
        want = oracle.bilstm_final(tok if rows is None else tok[rows], sd["word_embedding.weight"], lstm_of(sd), sd["lang_fc.weight"], sd["lang_fc.bias"])
        args = (dev(tok), dev(sd["word_embedding.weight"]), {k: dev(v) for k, v in lstm_of(sd).items()},
                dev(sd["lang_fc.weight"]), dev(sd["lang_fc.bias"]))
        _CASES[(H, B)] = (args, lens, torch.from_numpy(want))
    return _CASES[(H, B)]


def active_rows(lens, B):
    """Active GEMM rows per step: (forward, reverse).  Forward: all B + 1 rows (the all-pad row 0 and every query).  Reverse:
    row 0 and the queries that have reached a real token, 1 + #{len > T - 1 - s} (rows are sorted by length, a prefix)."""
    return [B + 1] * T, [1 + int((lens > T - 1 - s).sum()) for s in range(T)]


def expected_blocks(lens, B, H, live, rows):
    """(16-row x 16-unit) blocks with matrix work per direction.  Live: blocks with a row below the active count and a unit
    below H -- independent of the tile height.  Not live: every block of every launched tile (tiles of `rows` rows that start
    below the active count, two 16-unit halves per 32-unit column tile)."""
    out = []
    for counts in active_rows(lens, B):
        if live:
            out.append(sum(-(-m // 16) * -(-H // 16) for m in counts))
        else:
            out.append(sum(-(-m // rows) * (rows // 16) * 2 * -(-H // 32) for m in counts))
    return tuple(out)


def run(vfr, args, H, B, live, tile=0, multi=0, count=False):
    ws = vfr.bilstm_workspace(B, T, E, H, VOCAB, DEV) if count else None
    old = {name: vfr.get_option(name) for name in ("lstm_live_blocks", "lstm_tile", "lstm_multi")}
    try:
        vfr.set_option("lstm_live_blocks", (1 if live else 0) | (2 if count else 0))
        vfr.set_option("lstm_tile", tile)
        vfr.set_option("lstm_multi", multi)
        out = vfr.bilstm_final(*args, workspace=ws)
        torch.cuda.synchronize()
        taken = vfr.get_option("lstm_multi_taken")
    finally:
        for name, value in old.items():
            vfr.set_option(name, value)
    assert vfr.poll_faults() == 0
    blocks = vfr.lstm_issued_blocks(ws, B, T, E, H, VOCAB) if count else None
    return out.cpu(), blocks, taken


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("H", HS)
def test_live_blocks_same_bits_per_step(vfr, oracle, H, B):
    """Per-step launches at every tile height: `lstm_live_blocks` 1 against 0 and against the oracle, bit for bit."""
    args, lens, want = case(H, B, oracle)
    for tile in TILES:
        ref, _, _ = run(vfr, args, H, B, live=False, tile=tile)
        got, _, taken = run(vfr, args, H, B, live=True, tile=tile)
        assert taken == 0
        assert torch.equal(got, ref), (H, B, tile)
        assert torch.equal(got, want), (H, B, tile)


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("H", HS)
def test_issued_blocks_match_the_lengths(vfr, oracle, H, B):
    """The debug counter (workspace, option bit 1) holds the blocks the steps issued matrix work for: with the skip exactly the
    live ones computed here from the lengths, whatever the tile height; without it every block of every launched tile, which is
    more -- so the skip happens.  Counting changes no bits."""
    args, lens, want = case(H, B, oracle)
    for tile in TILES:
        rows = TILE_ROWS[tile] if tile else 32              # by size: up to 700 rows run 32-row tiles
        got, blocks, _ = run(vfr, args, H, B, live=True, tile=tile, count=True)
        full, blocks_full, _ = run(vfr, args, H, B, live=False, tile=tile, count=True)
        exp, exp_full = expected_blocks(lens, B, H, True, rows), expected_blocks(lens, B, H, False, rows)
        print(f"H={H} B={B} tile={tile}: issued {blocks} expected {exp}; without the skip {blocks_full} expected {exp_full}")
        assert blocks == exp, (H, B, tile)
        assert blocks_full == exp_full, (H, B, tile)
        assert exp[0] <= exp_full[0] and exp[1] < exp_full[1], (H, B, tile)     # (the reverse prefix always ends mid-tile somewhere)
        assert torch.equal(got, want) and torch.equal(full, want), (H, B, tile)


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("H", HS)
def test_live_blocks_same_bits_one_launch(vfr, oracle, H, B):
    """The one-launch sequence kernel (`lstm_multi` 1; tile by size and 128 rows, as its parity test runs it): the same counts per
    task, the same bits.  Where the launch-time residency check declines the launch the per-step launches must have been taken and
    give the same bits; the case is then reported as skipped."""
    args, lens, want = case(H, B, oracle)
    declined = False
    for tile in (0, 2):
        ref, _, _ = run(vfr, args, H, B, live=False, tile=tile, multi=1)
        got, blocks, taken = run(vfr, args, H, B, live=True, tile=tile, multi=1, count=True)
        assert torch.equal(got, ref), (H, B, tile)
        assert torch.equal(got, want), (H, B, tile)
        assert blocks == expected_blocks(lens, B, H, True, 0), (H, B, tile)     # per-step fallback or one launch: the same blocks
        assert taken in (1, 2), (H, B, tile, taken)        # selected at these shapes: 1 = ran, 2 = declined by the residency check
        declined |= taken == 2
    if declined:
        pytest.skip("the one-launch kernel's grid is not resident at once on this device: per-step launches taken, same bits")


AUTO_ROWS = np.r_[0:24, 2400:2424]


@pytest.mark.parametrize("H,B,tile,expect", [(512, 2499, 0, 1), (512, 2498, 0, 0), (480, 2499, 0, 0), (512, 2499, 1, 0)])
def test_automatic_form_selection(vfr, oracle, H, B, tile, expect):
    """The shipped default, `lstm_multi` 2: the one-launch kernel (128-row tiles) from `lstm_multi_min` = 2 500 GEMM rows (queries
    + 1) on at H >= 512 while no tile height is forced; one row fewer, H = 480 or `lstm_tile` 1 take the per-step launches.
    Either way the bits of `lstm_multi` 0 and, on a slice of the batch (rows are encoded independently), of the oracle."""
    assert vfr.get_option("lstm_multi_min") == 2500
    args, lens, want = case(H, B, oracle, rows=AUTO_ROWS)
    ref, _, taken0 = run(vfr, args, H, B, live=True, tile=tile, multi=0)
    got, blocks, taken = run(vfr, args, H, B, live=True, tile=tile, multi=2, count=True)
    assert taken0 == 0
    assert taken == expect or (expect == 1 and taken == 2), (H, B, tile, taken)     # (2: selected, grid not resident at once)
    assert torch.equal(got, ref), (H, B, tile)
    assert torch.equal(got[torch.from_numpy(AUTO_ROWS)], want), (H, B, tile)
    assert blocks == expected_blocks(lens, B, H, True, 0), (H, B, tile)
    with pytest.raises(RuntimeError, match="read-only"):
        vfr.set_option("lstm_multi_taken", 1)
