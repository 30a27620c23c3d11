"""The streaming resampler without a GPU: the host schedule of ``LogMelStream(resample=...)`` (which 16 kHz samples, rows and
examples a push of input frames completes) against the offline definitions on the whole signal, the rings emulated from the
very tables a push uploads (holding sample *indices* instead of values, so every check is integer-exact), the ring sizes the
module derives, and every refusal that must come before a launch."""
import ctypes
import random

import numpy as np
import pytest
import torch

WIN, HOP = 96, 100 / 30
CONFIGS = ((48000, 1), (44100, 1), (22050, 1), (8000, 1), (192000, 1), (16000, 2))
FILTERS = ("kaiser_best", "kaiser_fast")
POS_MOD = 1 << 30


def _mod():
    from feature_vs_text_compound_emotion_amd import audio_stream
    return audio_stream


def _table(rate, filter):
    from feature_vs_text_compound_emotion_amd.audio_backbone import resample_taps
    taps, L, M = resample_taps(rate, filter)
    return L, M, taps.shape[1]


def _lengths(rate, T):
    """Eight signal lengths in input frames: none, one, around the filter's reach (shorter than J + 2 frames: no output before
    ``finish``), around one STFT row, and two that give examples before ``finish``."""
    J = (T - 2) // 2
    return (0, 1, J + 1, J + 2, J + 3 + 400 * rate // 16000, rate // 7 + 3, int(1.05 * rate) + 1, int(1.31 * rate))


def _chunks(n, max_samples, rng):
    out = []
    while n:
        out.append(min(n, rng.randint(1, max_samples)))
        n -= out[-1]
    return out


class Rings:
    """The three rings of one stream, holding indices: in[slot] = the input frame written there, out[slot] = the 16 kHz
    sample, mel[slot] = the row.  ``run`` does to them what the four kernels do, from the int32 tables alone."""

    def __init__(self, rin, rs, rm, L, M, T):
        self.rin, self.rs, self.rm, self.L, self.M, self.T = rin, rs, rm, L, M, T
        self.inp, self.out, self.mel = np.full(rin, -1, np.int64), np.full(rs, -1, np.int64), np.full(rm, -1, np.int64)
        self.frames = self.produced = self.rows = 0       # unwrapped counters, for the expected indices only

    def run(self, mix_t, out_t, row_t, ex_t, win):
        L, M, T = self.L, self.M, self.T
        J = (T - 2) // 2
        if mix_t is not None:
            (_, pos, count, off), = mix_t.t().tolist()
            slots = (pos + np.arange(count)) & (self.rin - 1)
            assert pos == self.frames % POS_MOD and count <= self.rin - (T - 1)
            if off < 0:
                assert self.inp[(pos - 1) & (self.rin - 1)] == self.frames - 1     # the frame a repeat copies is still there
            self.inp[slots] = self.frames + np.arange(count)
            self.frames += count
        if out_t is not None:
            (_, n0, count, r0, pos_q0, lo, hi), = out_t.t().tolist()
            n_abs = self.produced + np.arange(count)                                # the outputs this segment must be
            assert n0 == self.produced % POS_MOD and 0 <= r0 < L
            num = r0 + np.arange(count, dtype=np.int64) * M                         # the kernel's 64-bit r0 + i M
            q_rel, row = num // L, num % L
            # against unbounded ints: the tap row and the centre of every output
            q_abs = np.array([(int(n) * M) // L for n in n_abs])
            assert [int(r) for r in row] == [(int(n) * M) % L for n in n_abs]
            k = q_rel[:, None] - J + np.arange(T)[None, :]                          # relative to q0, as the kernel walks
            valid = (k >= max(lo, hi - self.rin)) & (k < hi)
            want = q_abs[:, None] - J + np.arange(T)[None, :]                       # the indices q - J .. q + J + 1
            in_signal = (want >= 0) & (want < self.frames)
            assert np.array_equal(valid, in_signal)                                 # out of range <=> answered by the check
            got = self.inp[(pos_q0 + k) & (self.rin - 1)]
            assert np.array_equal(got[valid], want[valid])                          # no slot stale or overwritten
            self.out[(n0 + np.arange(count)) & (self.rs - 1)] = n_abs
            self.produced += count
        for _, pos, r in (row_t.t().tolist() if row_t is not None else []):
            assert r == self.rows % POS_MOD
            want = 160 * self.rows + np.arange(400)
            assert pos == want[0] % POS_MOD and want[-1] < self.produced
            assert np.array_equal(self.out[(pos + np.arange(400)) & (self.rs - 1)], want)
            self.mel[r & (self.rm - 1)] = self.rows
            self.rows += 1
        starts = []
        for _, start in (ex_t.t().tolist() if ex_t is not None else []):
            got = self.mel[(start + np.arange(win)) & (self.rm - 1)]
            assert np.array_equal(got, got[0] + np.arange(win)) and got[-1] < self.rows and got[0] % POS_MOD == start
            starts.append(int(got[0]))
        return starts


def _run(n, chunks, rate, filter, max_samples, emulate):
    """One signal of n input frames through the pure schedule the way ``push`` and ``finish`` drive it.  Returns (16 kHz
    samples before finish, starts before finish, all starts, final state); with ``emulate`` the tables of every push are
    built by ``ops.resample_stream_tables`` and run on index-holding rings."""
    from feature_vs_text_compound_emotion_amd import ops
    from feature_vs_text_compound_emotion_amd.audio_backbone import resampled_length
    a = _mod()
    L, M, T = _table(rate, filter)
    rin, rs, rm, max_out = a.resample_ring_sizes(WIN, max_samples, L, M, T)
    rings = Rings(rin, rs, rm, L, M, T) if emulate else None
    state, got = (0, 0, 0, 0), []

    def step(count, offset, limit, final):
        nonlocal state
        old = state
        state, mix, out, new_rows, starts = a.resampled_step(old, count, offset, L, M, T, WIN, HOP, limit, final)
        frames, produced, rows, _ = state
        assert frames == old[0] + count and produced - old[1] <= max_out and len(new_rows) <= rm
        assert (out is None) == (produced == old[1]) and (mix is None) == (count == 0)
        # the ring bounds, at every push: the oldest input a new output reads against the newest, and so on down the chain
        if out is not None:
            q_first = (old[1] * M) // L
            assert (frames - 1) - max(q_first - (T - 2) // 2, 0) <= rin - 1
            assert out[:2] == (old[1], produced - old[1]) and (out[3], out[2]) == divmod(old[1] * M, L) and out[4] == frames
        if new_rows:
            assert (produced - 1) - 160 * new_rows[0] <= rs - 1 and 160 * new_rows[-1] + 399 <= produced - 1
        if starts:
            assert (rows - 1) - starts[0] <= rm - 1 and starts[-1] + WIN <= rows
        if emulate and (mix is not None or out is not None):
            tables = ops.resample_stream_tables([(0,) + mix] if mix else [], [(0,) + out] if out else [],
                                                [(0, 160 * r, r) for r in new_rows], [(0, s) for s in starts], "cpu")
            assert rings.run(*tables, WIN) == starts
        got.extend(starts)

    assert sum(chunks) == n and all(1 <= c <= max_samples for c in chunks)
    at = 0
    for c in chunks:
        step(c, at, None, None)
        at += c
    produced_before, before = state[1], list(got)
    if n:
        final = resampled_length(n + rate, rate)
        limit = a.num_examples(a.num_rows(final), WIN, HOP)
        for c in a.pad_chunks(max_samples, rate):
            assert 1 <= c <= max_samples
            step(c, None, limit, None)
        assert state[0] == n + rate
        step(0, None, limit, final)
        assert state[1] == final
    return produced_before, before, got, state


@pytest.mark.parametrize("filter", FILTERS)
@pytest.mark.parametrize("rate,channels", CONFIGS)
def test_schedule_emits_the_offline_samples_rows_and_examples_under_any_chunking(rate, channels, filter):
    from feature_vs_text_compound_emotion_amd.audio_backbone import example_starts, resampled_length
    a = _mod()
    L, M, T = _table(rate, filter)
    J = (T - 2) // 2
    for n in _lengths(rate, T):
        complete = len([k for k in range(n * L // M + 2) if (k * M) // L + J + 1 < n])
        final = resampled_length(n + rate, rate) if n else 0
        full_ref = example_starts(a.num_rows(final), WIN, HOP) if n else []
        before_ref = [s for s in full_ref if s + WIN <= a.num_rows(complete)]
        cases = []
        for seed in range(20):
            ms = (100, 700, 4096)[seed % 3]
            cases.append((_chunks(n, ms, random.Random(1000 * seed + n)), ms))
        if n:
            cases.append(([n], n))                                  # one chunk
            cases.append(([37] * (n // 37) + ([n % 37] if n % 37 else []), 100))
        if 0 < n <= 1500:
            cases.append(([1] * n, 100))                            # one-frame ticks
        for chunks, ms in cases:
            produced, before, got, state = _run(n, chunks, rate, filter, ms, emulate=False)
            assert produced == complete, (rate, filter, n, ms)      # exactly {n : (n M) div L + J + 1 < S}
            assert got == full_ref and before == before_ref, (rate, filter, n, ms)
            if n:
                assert state == (n + rate, final, a.num_rows(final), len(full_ref))


@pytest.mark.parametrize("filter", FILTERS)
@pytest.mark.parametrize("rate,channels", CONFIGS)
def test_emulated_rings_hold_every_index_an_output_a_row_and_an_example_read(rate, channels, filter):
    """Every output reads exactly q - J .. q + J + 1: the ones inside the signal from slots that hold those very indices, the
    others answered by the range check.  Small pushes, so that every ring wraps many times."""
    L, M, T = _table(rate, filter)
    n = rate // 5 + 7
    for ms, seed in ((100, 1), (100, None), (257, 3), (4096, 4)):
        if seed is None:        # one-frame ticks
            n_case = min(n, 1200)
            chunks = [1] * n_case
        else:
            n_case, chunks = n, _chunks(n, ms, random.Random(seed))
        _, _, got, state = _run(n_case, chunks, rate, filter, ms, emulate=True)
        assert state[1] > 16000 and len(got) == state[3]


def test_ring_sizes_are_the_derived_powers_of_two():
    a = _mod()
    for rate, _ in CONFIGS:
        for filter in FILTERS:
            L, M, T = _table(rate, filter)
            for ms in (1, 100, 1600, 4096):
                rin, rs, rm, max_out = a.resample_ring_sizes(WIN, ms, L, M, T)
                assert max_out == max(ms * L // M + 1, (T // 2) * L // M + 2)
                assert rin & (rin - 1) == 0 and rin >= T - 1 + ms > rin // 2
                assert rs & (rs - 1) == 0 and rs >= 399 + max_out > rs // 2
                assert rm & (rm - 1) == 0 and rm >= WIN + max_out // 160 + 1 > rm // 2
    s = a.LogMelStream(3, 1 / 30, max_samples=1600, sample_rate=48000, channels=2, resample="kaiser_best")
    assert (s.L, s.M, s.T) == (1, 3, 386) and (s.ring_inputs, s.ring_samples, s.ring_rows) == (2048, 1024, 128)
    assert s.samples_seen == [0, 0, 0] and s.resampled == [0, 0, 0] and s.examples_emitted == [0, 0, 0]
    assert abs(s.delay_sec - 193 / 48000) < 1e-15 and round(s.delay_sec * 1e3, 1) == 4.0
    assert a.outputs_complete(193, 1, 3, 386) == 0 and a.outputs_complete(194, 1, 3, 386) == 1
    assert a.outputs_complete(197, 1, 3, 386) == 2


def test_tables_reduce_positions_modulo_2_30_and_pack_one_tensor():
    from feature_vs_text_compound_emotion_amd import ops
    big = 1 << 30
    mix, out, row, ex = ops.resample_stream_tables(
        [(1, big + 5, 7, 3), (2, 9, 4, None)], [(1, 3 * big + 11, 6, 2, 5 * big + 40, 5 * big + 90), (0, 0, 1, 0, 0, 3 * big)],
        [(0, 2 * big + 160, big + 1)], [(4, 3 * big + 2)], "cpu")
    assert mix.tolist() == [[1, 2], [5, 9], [7, 4], [3, -1]]
    # the valid range is relative to q0: [-q0, inputs - q0), each end clamped to +-2^30
    assert out.tolist() == [[1, 0], [11, 0], [6, 1], [2, 0], [40, 0], [-big, 0], [50, big]]
    assert row.tolist() == [[0], [160], [1]] and ex.tolist() == [[4], [2]]
    assert mix.dtype == torch.int32
    assert mix.untyped_storage().data_ptr() == ex.untyped_storage().data_ptr() == out.untyped_storage().data_ptr()
    assert ops.resample_stream_tables([(0, 0, 1, 0)], [], [], [], "cpu")[1:] == (None, None, None)
    for bad in (([(0, 0, 0, 0)], []), ([(0, -1, 1, 0)], []), ([], [(0, 0, 0, 0, 0, 0)]), ([], [(0, 0, 1, -1, 0, 0)])):
        with pytest.raises(ValueError):
            ops.resample_stream_tables(*bad, [], [], "cpu")


def test_c_entries_refuse_before_any_launch():
    from feature_vs_text_compound_emotion_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)    # never dereferenced: every call below is refused on the host

    def refused(rc, name):
        assert rc == -1 and lib.cer_last_error().startswith(name), (rc, lib.cer_last_error())

    def append(packed=p, seg=p, ring=p, rin=2048, n=1, c=2, a=1, mc=1, hist=385, s=1):
        return lib.cer_resample_stream_append(packed, n, c, seg, a, mc, hist, ring, s, rin, None)

    def outputs(inr=p, seg=p, taps=p, out=p, rin=2048, rs=1024, a=1, mc=1, L=1, M=3, T=386, s=1):
        return lib.cer_resample_stream_outputs(inr, s, rin, seg, a, mc, taps, L, M, T, out, rs, None)

    def rows(ring=p, tab=p, mel=p, out=p, rs=1024, rm=128, n=1, s=1):
        return lib.cer_logmel_stream_rows_f64(ring, s, rs, tab, n, mel, 0.01, out, rm, None)

    for kw in ({"packed": None}, {"seg": None}, {"ring": None}, {"n": 0}, {"c": 0}, {"a": 0}, {"mc": 0}, {"s": 0}, {"hist": -1},
               {"mc": 2048}, {"mc": 1664}, {"hist": 2048}, {"a": 65536}):
        refused(append(**kw), b"resample_stream_append")       # mc = 1664: 385 old inputs + 1664 new ones > Rin = 2048
    for kw in ({"inr": None}, {"seg": None}, {"taps": None}, {"out": None}, {"a": 0}, {"mc": 0}, {"s": 0}, {"L": 0}, {"M": 0},
               {"L": -1}, {"M": -3}, {"T": 0}, {"T": 1}, {"T": 385}, {"T": -2}, {"rin": 256}, {"mc": 1025}, {"a": 65536},
               {"M": 1 << 30}, {"T": 1 << 24, "rin": 1 << 25}):
        refused(outputs(**kw), b"resample_stream_outputs")     # rin = 256 < T; 256 M / L + T inputs per block over 2^24
    for kw in ({"ring": None}, {"tab": None}, {"mel": None}, {"out": None}, {"n": 0}, {"s": 0}, {"rs": 256}):
        refused(rows(**kw), b"logmel_stream_rows_f64")
    for bad in (0, 399, 1000, 1 << 31, -1024):
        refused(append(rin=bad), b"resample_stream_append")
        refused(outputs(rin=bad), b"resample_stream_outputs")
        refused(outputs(rs=bad), b"resample_stream_outputs")
        refused(rows(rs=bad), b"logmel_stream_rows_f64")
        refused(rows(rm=bad), b"logmel_stream_rows_f64")


def test_constructor_and_push_refuse_bad_arguments():
    a = _mod()
    ok = {"streams": 2, "hop_sec": 0.025, "sample_rate": 48000, "channels": 2, "resample": "kaiser_fast"}
    for kw in ({"resample": "sinc_best"}, {"resample": "linear"}, {"channels": 0}, {"channels": -1}, {"channels": 1.5},
               {"sample_rate": 0}, {"sample_rate": -48000}, {"sample_rate": 44100.5}, {"sample_rate": 47999, "resample": "kaiser_best"},
               {"hop_sec": 0.005}, {"streams": 0}, {"max_samples": 0}, {"device": "cpu"},
               {"resample": None}, {"resample": None, "sample_rate": 16000}):     # 2 channels need a filter, at 16 kHz too
        with pytest.raises(ValueError):
            a.LogMelStream(**{**ok, **kw})
    with pytest.raises(ValueError, match="MAX_RESAMPLE_TAPS|tap table"):
        a.LogMelStream(1, 0.025, sample_rate=47999, resample="kaiser_best")     # L = 16000, T = 386: over the table limit
    with pytest.raises(ValueError, match="wav_int16_to_examples"):
        a.LogMelStream(2, 0.025, sample_rate=48000)                              # as before without resample=
    s = a.LogMelStream(2, 0.025, max_samples=100, sample_rate=48000, channels=2, resample="kaiser_fast")
    pcm = torch.zeros((30, 2), dtype=torch.int16)
    for bad_pcm, counts in ((pcm, [30]), (pcm, [10, 10, 10]), (pcm, [-1, 31]), (pcm[:1].repeat(101, 1), [101, 0]),
                            (pcm, [10, 10]), (pcm, [20, 20]), (pcm.float(), [10, 20]), (pcm.int(), [10, 20]),
                            (pcm[:, 0], [10, 20]), (pcm.view(20, 3), [10, 10]), (pcm.view(30, 2, 1), [10, 20]),
                            (pcm.view(60), [20, 40]), (np.zeros((30, 2), np.float32), [10, 20]), (pcm, 30)):
        with pytest.raises(ValueError):
            s.push(bad_pcm, counts)
    assert s.samples_seen == [0, 0] and s.resampled == [0, 0] and s.rows_done == [0, 0] and s.examples_emitted == [0, 0]
    assert s._ring is None and s._inring is None and s._taps is None      # nothing was allocated, nothing launched
    mono = a.LogMelStream(1, 0.025, max_samples=100, sample_rate=8000, resample="kaiser_fast")
    with pytest.raises(ValueError):
        mono.push(torch.zeros((10, 2), dtype=torch.int16), [10])
    assert mono._ring is None
    with pytest.raises(IndexError):
        s.reset([2])
