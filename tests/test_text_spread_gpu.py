"""``ops.text_spread_rows`` / ``cer_text_spread_rows`` against the index composition on the host: row out_first + i of a segment
is row ``token_rows[align_tokens_to_frames(n_tokens, n_frames)[i]]`` of the token matrix, zeros without a token, and nothing
else is written.  A row copy: every comparison is for equality."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 5      # rows of NaN before and after every buffer the kernel writes
TOK_ROWS = 23
# (n_tokens, n_frames): no token, one of each, exact, tokens dropped, blocks of unequal length, one token over two waves' worth
SHAPES = [(0, 3), (1, 1), (5, 5), (7, 3), (3, 7), (4, 10), (1, 65)]


@functools.lru_cache(maxsize=None)
def _tok(hidden):
    g = torch.Generator().manual_seed(hidden)
    return torch.randn((TOK_ROWS, hidden), generator=g).cuda()


def _segments():
    """The seven shapes in one launch: a gap of 2 uncovered rows before every second segment, out of output order, token rows
    non-contiguous and repeated."""
    g, segments, at = torch.Generator().manual_seed(3), [], 1
    for k, (n_tokens, n_frames) in enumerate(SHAPES):
        at += 2 * (k % 2)
        rows = torch.randint(0, TOK_ROWS, (n_tokens,), generator=g).tolist()
        if n_tokens >= 4:
            rows[2] = rows[0]      # a repeated row
        segments.append((at, n_frames, rows))
        at += n_frames
    order = [3, 0, 6, 1, 5, 2, 4]
    return [segments[i] for i in order], at + 3      # three uncovered rows at the end


def _want(tok, segments, out_rows):
    """(expected rows, covered mask) on the host's index plan."""
    from feature_vs_text_compound_emotion_amd.feature_extractor import align_tokens_to_frames
    want = torch.zeros((out_rows, tok.shape[1]), device=tok.device)
    covered = torch.zeros(out_rows, dtype=torch.bool, device=tok.device)
    for first, n_frames, rows in segments:
        covered[first:first + n_frames] = True
        for i, j in enumerate(align_tokens_to_frames(len(rows), n_frames)):
            want[first + i] = tok[rows[j]]
    return want, covered


def _guarded(rows, hidden):
    buf = torch.full((rows + 2 * GUARD, hidden), float("nan"), device="cuda")
    return buf, buf[GUARD:GUARD + rows]


@pytest.mark.parametrize("hidden", [4, 768])
def test_spread_equals_the_host_index_plan_and_writes_nothing_else(hidden):
    from feature_vs_text_compound_emotion_amd import ops
    tok = _tok(hidden)
    segments, out_rows = _segments()
    want, covered = _want(tok, segments, out_rows)
    assert (~covered).sum().item() == 1 + 2 * 3 + 3
    buf, out = _guarded(out_rows, hidden)
    got = ops.text_spread_rows(tok, segments, out_rows, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(out[covered], want[covered])
    assert torch.isnan(out[~covered]).all()                                  # uncovered rows are not written
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + out_rows:]).all()
    fresh = ops.text_spread_rows(tok, segments, out_rows)                    # a fresh output: uncovered rows are zeros
    assert fresh.shape == (out_rows, hidden) and torch.equal(fresh, want)


def test_more_frames_than_one_pass_of_the_grid():
    """One token over 300 frames and 9 over 1000: the waves of a segment stride over its frames more than once
    (64 blocks x 4 waves = 256 frames per pass)."""
    from feature_vs_text_compound_emotion_amd import ops
    tok = _tok(8)
    segments = [(1000, 300, [7]), (0, 1000, [3, 1, 4, 1, 5, 9, 2, 6, 5])]
    want, covered = _want(tok, segments, 1300)
    assert covered.all()
    assert torch.equal(ops.text_spread_rows(tok, segments, 1300), want)


def test_wrapper_refusals_launch_nothing():
    from feature_vs_text_compound_emotion_amd import ops
    tok = _tok(4)
    buf, out = _guarded(6, 4)
    for segments in ([(0, 3, [0]), (2, 2, [1])], [(4, 3, [0])], [(0, 2, [TOK_ROWS])], [(0, 2, [-1])], [(0, 0, [])], []):
        with pytest.raises(ValueError):
            ops.text_spread_rows(tok, segments, 6, out=out)
    with pytest.raises(ValueError):
        ops.text_spread_rows(tok, [(0, 2, [0])], 6, out=out[:5])
    with pytest.raises(ValueError):
        ops.text_spread_rows(torch.zeros((3, 6), device="cuda"), [(0, 2, [0])], 6)
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()


# ---------------------------------------------------------------------------------------------- the raw entry
def _raw(tok, segments, index, out, hidden=None, n_segments=None, n_index=None, null=()):
    from feature_vs_text_compound_emotion_amd import _lib
    table = torch.tensor([v for seg in segments for v in seg] + list(index), dtype=torch.int32).cuda()
    g = len(segments)
    args = {"tok": _lib.ptr(tok), "segments": _lib.ptr(table[:4 * g]), "tok_index": _lib.ptr(table[4 * g:]), "out": _lib.ptr(out)}
    for name in null:
        args[name] = None
    lib = _lib.load()
    rc = lib.cer_text_spread_rows(args["tok"], tok.shape[0], tok.shape[1] if hidden is None else hidden, args["segments"],
                                  g if n_segments is None else n_segments, args["tok_index"],
                                  len(index) if n_index is None else n_index, args["out"], out.shape[0], _lib.current_stream())
    return rc, lib.cer_last_error().decode()


def test_tables_the_host_did_not_check_stay_inside_the_buffers():
    """The entry cannot read its tables, so the kernel clamps what they hold (csrc/text_spread.hip: the frames of a segment
    are cut to the output rows [0, out_rows), the index position is clamped into [0, n_index), the token row into
    [0, tok_rows)).  A table with a token row of -7 and of tok_rows + 100, index_first far outside the index table and
    segments that start before row 0 and end after the last row gives rows of ``tok`` or zeros inside the output, and
    touches nothing outside it."""
    hidden, out_rows = 8, 14
    tokbuf, tok = _guarded(TOK_ROWS, hidden)      # the token matrix inside NaN guards too: a read outside it would show
    tok.copy_(_tok(8))
    buf, out = _guarded(out_rows, hidden)
    index = [-7, TOK_ROWS + 100, 4, 2 ** 31 - 1, -2 ** 31]
    last = TOK_ROWS - 1
    segments = [(-3, 5, 1, 2),                  # starts before row 0: only its frames 3 and 4 land, at rows 0 and 1 (token row 4)
                (2, 2, 2, 0),                   # token rows -7 and tok_rows + 100: clamped to rows 0 and tok_rows - 1
                (4, 2, 2, 2 ** 31 - 2),         # index_first past the table: its last entry (-2^31 -> row 0), twice
                (6, 2, 2, -50),                 # index_first before the table: entry 0 (-7 -> row 0), twice
                (8, -4, 3, 0),                  # a negative frame count: nothing
                (9, 2, -3, 0),                  # a negative token count: zeros
                (12, 2 ** 31 - 1, 1, 2),        # runs past the last row: rows 12 and 13 get token row 4
                (2 ** 31 - 1, 2 ** 31 - 1, 1, 2)]   # entirely outside
    want = [4, 4, 0, last, 0, 0, 0, 0, None, "zeros", "zeros", None, 4, 4]
    rc, err = _raw(tok, segments, index, out)
    assert rc == 0, err
    torch.cuda.synchronize()
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + out_rows:]).all()
    assert torch.isnan(tokbuf[:GUARD]).all() and torch.isnan(tokbuf[GUARD + TOK_ROWS:]).all()
    for r, w in enumerate(want):
        if w is None:
            assert torch.isnan(out[r]).all(), r
        else:
            assert torch.equal(out[r], torch.zeros_like(out[r]) if w == "zeros" else tok[w]), r


def test_entry_refusals():
    tok = _tok(4)
    buf, out = _guarded(4, 4)
    seg, index = [(0, 2, 1, 0)], [0]
    wide = torch.zeros((4, 6), device="cuda")
    rc, err = _raw(wide, seg, index, out, hidden=6)
    assert rc == -1 and "text_spread_rows" in err and "multiple of 4" in err
    for name in ("tok", "segments", "tok_index", "out"):
        rc, err = _raw(tok, seg, index, out, null=(name,))
        assert rc == -1 and "text_spread_rows: null pointer" in err, name
    for kw in (dict(hidden=0), dict(n_segments=0), dict(n_index=0), dict(n_segments=-1)):
        rc, err = _raw(tok, seg, index, out, **kw)
        assert rc == -1 and "text_spread_rows" in err, kw
    rc, err = _raw(tok, seg, index, out[:0])
    assert rc == -1 and "text_spread_rows" in err
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()
