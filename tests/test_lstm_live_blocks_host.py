"""Host-side plan of the fused BiLSTM steps (`vfr_lstm_plan`, no GPU): which batches take the one-launch kernel, with which
tile height and grid.  `lstm_multi` 2 (the default) = automatic: from `lstm_multi_min` GEMM rows (queries + 1) on, at H >= 512, with
128-row tiles, unless `lstm_tile` forces a height; 1 = wherever the shape is supported, tile height as the per-step launch picks
it; 0 = never.  The cross-check switches of the per-step launch select the per-step launches."""
import pytest

CUS, T = 256, 20


@pytest.fixture()
def vfr():
    from vfr_amd import _vfr
    _vfr.lib()
    names = ("lstm_multi", "lstm_multi_min", "lstm_tile", "lstm_fast", "lstm_skip0", "lstm_xcd")
    old = {n: _vfr.get_option(n) for n in names}
    for n, v in zip(names, (2, 2500, 0, 1, 1, 1)):        # the shipped values, whatever earlier tests of the process left behind
        _vfr.set_option(n, v)
    yield _vfr
    for n, v in old.items():
        _vfr.set_option(n, v)


def test_shipped_defaults():
    """Options are process-global and other tests set them: the defaults are read in a fresh process."""
    import subprocess
    import sys
    from pathlib import Path
    code = ("from vfr_amd import _vfr; print([_vfr.get_option(n) for n in "
            "('lstm_multi', 'lstm_multi_min', 'lstm_live_blocks', 'lstm_tile')], _vfr.lstm_plan(5001, 1000, 20, 256))")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=Path(__file__).resolve().parent.parent)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "[2, 2500, 1, 0] (True, 2, 512)"


def test_automatic_selection_thresholds(vfr):
    # the bench shape: 5 001 rows, H = 1000 -> one launch, 128-row tiles, two workgroups per CU in whole groups of eight
    assert vfr.lstm_plan(5001, 1000, T, CUS) == (True, 2, 512)
    assert vfr.lstm_plan(2500, 1000, T, CUS) == (True, 2, 512)
    assert vfr.lstm_plan(2499, 1000, T, CUS) == (False, 1, 0)          # below lstm_multi_min: per-step launches, 64-row tiles
    assert vfr.lstm_plan(700, 1000, T, CUS) == (False, 3, 0)           # ... 32-row tiles up to 700 rows
    assert vfr.lstm_plan(701, 1000, T, CUS) == (False, 1, 0)
    assert vfr.lstm_plan(5001, 512, T, CUS)[0] and not vfr.lstm_plan(5001, 480, T, CUS)[0]      # every XCD group needs column tiles
    assert not vfr.lstm_plan(5001, 1056, T, CUS)[0]                    # H <= 1024
    assert not vfr.lstm_plan(5001, 1012, T, CUS)[0]                    # remainder of the recurrent segment over 8: general K-loop
    vfr.set_option("lstm_multi_min", 1000)
    assert vfr.lstm_plan(1000, 1000, T, CUS) == (True, 2, 512) and not vfr.lstm_plan(999, 1000, T, CUS)[0]


def test_forced_tile_and_cross_checks_take_the_per_step_launches(vfr):
    for tile in (1, 2, 3):
        vfr.set_option("lstm_tile", tile)
        assert vfr.lstm_plan(5001, 1000, T, CUS) == (False, tile, 0)
    vfr.set_option("lstm_tile", 0)
    for opt in ("lstm_fast", "lstm_skip0", "lstm_xcd"):
        vfr.set_option(opt, 0)
        assert not vfr.lstm_plan(5001, 1000, T, CUS)[0], opt
        vfr.set_option(opt, 1)
    vfr.set_option("lstm_multi", 0)
    assert vfr.lstm_plan(5001, 1000, T, CUS) == (False, 1, 0)


def test_always_mode_follows_the_per_step_tile(vfr):
    vfr.set_option("lstm_multi", 1)
    assert vfr.lstm_plan(5001, 1000, T, CUS) == (True, 1, 768)         # 64-row tiles, three workgroups per CU
    assert vfr.lstm_plan(301, 1000, T, CUS) == (True, 3, 768)          # 32-row tiles up to 700 rows
    assert vfr.lstm_plan(33, 96, 2, CUS) == (True, 3, 2 * 2 * 8 * 2)       # small grids: no more slots than tasks (2 directions x 2 row tiles x 8 groups x T)
    vfr.set_option("lstm_tile", 2)
    assert vfr.lstm_plan(5001, 1000, T, CUS) == (True, 2, 512)
    assert vfr.lstm_plan(5001, 1000, T, 4) == (True, 2, 8)             # never fewer than one workgroup per XCD group
    assert not vfr.lstm_plan(5001, 1002, T, CUS)[0]                    # H % 4


def test_taken_report_is_read_only(vfr):
    with pytest.raises(RuntimeError, match="read-only"):
        vfr.set_option("lstm_multi_taken", 1)
