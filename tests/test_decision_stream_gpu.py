"""``DecisionStream`` on the GPU against ``decision_ref`` (the float64 mirror of ``metrics.format_trg_pred_video``), against the
offline ``video_confusion_kernel`` and against itself under every way of cutting a stream into pushes.

What is compared how (decision_ref's constants):
  vote, mean-logit decision, mean_outputs   exactly: the vote is integer work, and the kernel's column sum is the mirror's
        chain (float64 adds of the float32 logits in time order), so the float64 means are the same bits on both sides;
  mean_probs      within PROB_TOL = 2e-6: the kernel's probabilities are float32 (expf, a <= 16-term float32 denominator);
  mean-probability decision   on every row where the mirror's top two means are >= GAP = 1e-5 apart.  On the seeded sequences
        at most SKIP_CAP = 1 % of the rows may fall below that (the CPU test asserts the same by the mirror alone).  The tie
        cases of ``eval_ref`` are built from equal vote counts, which are ties of the probability means in real arithmetic: there
        the rule is applied without the cap.
Measured maxima are printed before each assertion."""
import functools

import numpy as np
import pytest
import torch

import decision_ref as ref
import eval_ref

pytestmark = pytest.mark.gpu


def _cls():
    from feature_vs_text_compound_emotion_amd import DecisionStream
    return DecisionStream


def _f32(a):
    return torch.from_numpy(np.asarray(a).astype(np.float32))


def _same(a, b):
    """Bitwise-equal values, NaN matching NaN."""
    a, b = a.cpu(), b.cpu()
    if not a.is_floating_point():
        return torch.equal(a, b)
    return a.shape == b.shape and torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(0.0, 1e30, -1e30), b.nan_to_num(0.0, 1e30, -1e30))


def _run(ds, seqs, ticks, fed=None):
    """Push the ticks (counts per stream) of the per-stream sequences ``seqs`` (numpy [T, C]) with ``track=True``.  Returns the
    per-stream tracks [(decisions, mean_outputs, mean_probs)] on the host, and the rows fed per stream."""
    fed = [0] * len(seqs) if fed is None else list(fed)
    parts = [[] for _ in seqs]
    for counts in ticks:
        if not sum(counts):
            assert ds.push_ragged(torch.empty((0, ds.n_out), device="cuda"), counts) is None
            continue
        rows = torch.from_numpy(np.concatenate([z[f:f + c] for z, f, c in zip(seqs, fed, counts)])).cuda()
        out, at = ds.push_ragged(rows, counts, track=True), 0
        for s, c in enumerate(counts):
            if c:
                parts[s].append(tuple(None if t is None else t[at:at + c].cpu() for t in out))
            at += c
        fed = [f + c for f, c in zip(fed, counts)]
    tracks = []
    for p in parts:
        tracks.append(tuple(None if not p or p[0][i] is None else torch.cat([q[i] for q in p]) for i in range(3)))
    return tracks, fed


def _chunks(total, n):
    return [min(n, total - t) for t in range(0, total, n)]


def _alone(z, chunk=None, **kw):
    """One stream alone in a fresh DecisionStream, pushed ``chunk`` rows at a time (default: in one push)."""
    chunk = len(z) if chunk is None else chunk
    kw.setdefault("max_new", chunk)
    ds = _cls()(z.shape[1], 1, **kw)
    tracks, _ = _run(ds, [z], [[c] for c in _chunks(len(z), chunk)])
    return tracks[0], ds


def _equal_tracks(a, b):
    return all((x is None and y is None) or _same(x, y) for x, y in zip(a, b)) and (a[0] is None or torch.equal(a[0], b[0]))


def _check_against_mirror(name, got, want, nc, cap):
    dec, mo, mp = got
    wd = torch.from_numpy(want["decisions"]).to(torch.int32)
    assert torch.equal(dec[:, 0], wd[:, 0]), f"{name}: vote"
    assert _same(mo[:, :nc], _f32(want["mean_outputs"])), f"{name}: mean logits"
    assert torch.equal(dec[:, 1], wd[:, 1]), f"{name}: mean-logit decision"
    wp = torch.from_numpy(want["mean_probs"])
    assert torch.equal(mp[:, :nc].isnan(), wp.isnan()), f"{name}: NaN pattern of the mean probabilities"
    err = (mp[:, :nc].double() - wp).abs().nan_to_num(0.0).max().item()
    clear = torch.from_numpy(want["gap"] >= ref.GAP)
    share = 1.0 - clear.double().mean().item()
    print(f"{name}: max |mean_probs - mirror| = {err:.3g}; rows below the gap: {share:.4f}")
    assert err <= ref.PROB_TOL, (name, err)
    assert torch.equal(dec[clear, 2], wd[clear, 2]), f"{name}: mean-probability decision"
    if cap:
        assert share <= ref.SKIP_CAP, (name, share)


# ---------------------------------------------------------------------------------------------- 1. every prefix
@functools.lru_cache(maxsize=None)
def _mirror(kind, key, window=None, drop_last=False):
    z = ref.prefix_sequence(key) if kind == "seq" else ref.stream_sequences()[key] if kind == "stream" else ref.eval_video(kind, key)
    return ref.track(z, window=window, drop_last=drop_last)


@pytest.mark.parametrize("name,streams", [("c2", 1), ("c7", 3), ("c8", 5), ("c16", 3)])
def test_every_prefix_of_a_seeded_sequence_equals_the_mirror(name, streams):
    z = ref.prefix_sequence(name)
    seqs = [z if s == streams - 1 else np.ascontiguousarray(z[::-1]) for s in range(streams)]   # the neighbours see other rows
    ds = _cls()(z.shape[1], streams, max_new=7)
    tracks, _ = _run(ds, seqs, [[c] * streams for c in _chunks(len(z), 7)])
    _check_against_mirror(name, tracks[-1], _mirror("seq", name), z.shape[1], cap=True)
    dec, mo, mp = ds.decide()
    assert torch.equal(dec[-1].cpu(), tracks[-1][0][-1]) and torch.equal(mo[-1].cpu(), tracks[-1][1][-1])
    assert torch.equal(mp[-1].cpu(), tracks[-1][2][-1])


@pytest.mark.parametrize("case,key", [("vote_ties", "tie_5_300_601"), ("vote_ties", "tie_300_5_601"), ("vote_ties", "majority_last"),
                                      ("equal_maxima", "two"), ("equal_maxima", "three"), ("equal_maxima", "all"),
                                      ("equal_maxima", "mixed")])
def test_every_prefix_of_the_tie_cases_equals_the_mirror(case, key):
    z = ref.eval_video(case, key)
    got, ds = _alone(z, chunk=32)
    _check_against_mirror(f"{case}/{key}", got, _mirror(case, key), z.shape[1], cap=False)
    want = eval_ref.get_case(case).video_preds[None][list(eval_ref.get_case(case).data).index(key)]
    assert ds.decide()[0][0].cpu().tolist() == want.tolist()       # the whole video: what the reference reports
    if key == "all":                                                # every column is the same column: index 0, three times
        assert got[0].unique().tolist() == [0]


# ---------------------------------------------------------------------------------------------- 2. the offline kernel
def _offline(case_data, n_cls, ic):
    from feature_vs_text_compound_emotion_amd.eval_device import DeviceEvalAccumulator
    logits = torch.from_numpy(np.concatenate([e["logits"] for e in case_data.values()])).cuda()
    labels = torch.from_numpy(np.concatenate([e["labels"] for e in case_data.values()])).cuda()
    off = np.cumsum([0] + [len(e["labels"]) for e in case_data.values()]).tolist()
    acc = DeviceEvalAccumulator(n_cls, ignore_classes=(ic,), keep_video_predictions=True)
    acc.add(logits, labels, video_offsets=off)
    return acc.video_predictions[0][1].cpu()


def _stream_videos(videos, n_cls, drop_last, streams=5, max_new=32):
    """Final ``decide()`` of every video: ``streams`` at a time, ragged, each stream reset before its next video."""
    ds, out = _cls()(n_cls, streams, max_new=max_new, drop_last=drop_last), []
    for v0 in range(0, len(videos), streams):
        batch = videos[v0:v0 + streams] + [videos[0][:0]] * (streams - len(videos[v0:v0 + streams]))
        left = [len(z) for z in batch]
        ticks = []
        while any(left):
            ticks.append([min(n, max_new) for n in left])
            left = [n - c for n, c in zip(left, ticks[-1])]
        ds.reset()
        fed = [0] * streams
        for counts in ticks:
            rows = torch.from_numpy(np.concatenate([z[f:f + c] for z, f, c in zip(batch, fed, counts)])).cuda()
            ds.push_ragged(rows, counts)
            fed = [f + c for f, c in zip(fed, counts)]
        out.append(ds.decide()[0][:len(videos[v0:v0 + streams])].cpu())
    return torch.cat(out)


@pytest.mark.parametrize("name", ["random_exact", "class_limits_c2", "class_limits_c16", "ignore_class"])
def test_final_decisions_equal_the_offline_accumulator(name):
    data, n_cls, ic = ref.offline_videos(name)
    exact = name != "ignore_class"
    videos = [e["logits"] for e in data.values()]
    want = _offline(data, n_cls, ic)
    got = _stream_videos(videos, n_cls, drop_last=ic is not None)
    assert torch.equal(got[:, 0], want[:, 0]), "vote"
    # exact videos: any float32 summation order is exact; the float videos of ``eval_ref`` keep their column means >= 1e-3
    # apart (``eval_ref.check_video``), which no summation order crosses
    assert torch.equal(got[:, 1], want[:, 1]), ("mean logits", exact)
    clear = torch.tensor([ref.decide(z, drop_last=ic is not None)[3] >= ref.GAP for z in videos])
    print(f"{name}: {int((~clear).sum())} of {len(videos)} videos below the gap")
    assert (~clear).double().mean().item() <= ref.SKIP_CAP
    assert torch.equal(got[clear, 2], want[clear, 2]), "mean probabilities"


# ---------------------------------------------------------------------------------------------- 3. chunking invariance
@functools.lru_cache(maxsize=None)
def _whole(s, window):
    """Stream ``s`` of the shared sequences alone, in one push: the track every other chunking must reproduce."""
    track, ds = _alone(ref.stream_sequences()[s], window=window)
    return track, tuple(t.cpu() for t in ds.decide())


@pytest.mark.parametrize("window", [None, 5])
def test_a_track_is_the_same_bits_however_the_stream_is_cut(window):
    z = ref.stream_sequences()[0]
    want, final = _whole(0, window)
    assert want[0].shape == (len(z), 3) and len(set(want[0][:, 2].tolist())) > 1
    for chunk, max_new in ((1, 32), (3, 3), (3, 32)):
        got, ds = _alone(z, chunk=chunk, max_new=max_new, window=window)
        assert _equal_tracks(got, want), (chunk, max_new)
        assert all(_same(a, b) for a, b in zip(ds.decide(), final)), (chunk, max_new)
    ds = _cls()(z.shape[1], 1, max_new=32, window=window)              # dense pushes longer than max_new: cut inside
    out = ds.push_rows(torch.tensor(z).cuda(), track=True)
    assert _equal_tracks(tuple(t.cpu() for t in out), want)
    _check_against_mirror(f"stream 0, window {window}", want, _mirror("stream", 0, window), z.shape[1], cap=True)


@pytest.mark.parametrize("window", [None, 5])
def test_five_ragged_streams_equal_each_stream_alone(window):
    seqs = list(ref.stream_sequences())
    ticks = ref.ragged_schedule([len(z) for z in seqs], 8, seed=3)
    ds = _cls()(ref.STREAM_C, 5, max_new=8, window=window)
    tracks, fed = _run(ds, seqs, ticks)
    assert fed == ds.frames_seen == [ref.STREAM_FRAMES] * 5
    final = ds.decide()
    for s in range(5):
        want, wfinal = _whole(s, window)
        assert _equal_tracks(tracks[s], want), s
        assert all(_same(a[s], b[0]) for a, b in zip(final, wfinal)), s


# ---------------------------------------------------------------------------------------------- 4. window mode
@pytest.mark.parametrize("max_new", ref.MAX_NEWS)
@pytest.mark.parametrize("window", ref.WINDOWS)
@pytest.mark.parametrize("start", [0, 2 ** 30 - 5])
def test_a_window_equals_a_fresh_whole_stream_fed_its_rows(window, max_new, start):
    seqs = list(ref.stream_sequences()[:3])
    ds = _cls()(ref.STREAM_C, 3, max_new=max_new, window=window)
    assert ds.state is None
    ds._pos = [start + s for s in range(3)]                             # the ring position crosses 2^30 after a few rows
    tracks, _ = _run(ds, seqs, ref.ragged_schedule([len(z) for z in seqs], max_new, seed=11 + window))
    r = ds.state["zring"].shape[1]
    assert r >= window + max_new and r // 2 < window + max_new and len(seqs[2]) >= 3 * r
    z = seqs[2]
    fresh = _cls()(ref.STREAM_C, 1, max_new=window)
    for t in range(len(z)):
        fresh.reset()
        out = fresh.push_rows(torch.tensor(z[max(0, t + 1 - window):t + 1]).cuda(), track=True)
        for got, want in zip(tracks[2], out):
            assert _same(got[t], want[-1].cpu()), (t, window, max_new)
    assert all(_same(a[2], b[0]) for a, b in zip(ds.decide(), fresh.decide()))


def test_whole_stream_counts_are_64_bit():
    """A stream that stands at 2^31 - 3 frames: the counts and ``first`` cross 2^31, the means divide by the 64-bit count."""
    z, start = ref.stream_sequences()[1][:40], 2 ** 31 - 3
    runs = []
    for chunk in (40, 3):
        ds = _cls()(ref.STREAM_C, 1, max_new=chunk)
        ds.frames_seen = [start]
        tracks, _ = _run(ds, [z], [[c] for c in _chunks(len(z), chunk)])
        runs.append((tracks[0], ds))
    (got, ds), (cut, _) = runs
    assert _equal_tracks(got, cut) and ds.frames_seen == [start + 40]
    want = ref.track(z, start=start)
    assert torch.equal(got[0][:, 0], torch.from_numpy(want["decisions"][:, 0]).to(torch.int32))
    assert torch.equal(got[1], _f32(want["mean_outputs"]))
    assert (got[2].double() - torch.from_numpy(want["mean_probs"])).abs().max().item() <= ref.PROB_TOL
    preds = np.argmax(z, axis=1)
    first = ds.state["first"][0].cpu().tolist()
    for c in range(ref.STREAM_C):
        seen = np.flatnonzero(preds == c)
        assert first[c] == (start + int(seen[0]) if len(seen) else 2 ** 63 - 1)
    assert max(f for f in first if f < 2 ** 63 - 1) >= 2 ** 31
    assert ds.state["votes"][0].cpu().tolist() == np.bincount(preds, minlength=ref.STREAM_C).tolist()


# ---------------------------------------------------------------------------------------------- 5. non-finite rows
NON_FINITE = ("nan_col0", "nan_middle", "pos_inf", "neg_inf", "overflow", "underflow", "both_inf", "plain")


@pytest.mark.parametrize("window", [None, 5])
@pytest.mark.parametrize("key", NON_FINITE)
def test_non_finite_rows_decide_as_the_mirror_does(key, window):
    z = ref.eval_video("non_finite", key)
    got, ds = _alone(z, chunk=32, window=window)
    want = _mirror("non_finite", key, window)
    _check_against_mirror(f"non_finite/{key}/window {window}", got, want, 7, cap=False)
    if window is None:
        case = eval_ref.get_case("non_finite")
        assert ds.decide()[0][0].cpu().tolist() == case.video_preds[None][list(case.data).index(key)].tolist()


def test_a_nan_stays_until_reset_and_leaves_a_window_with_its_row():
    z = ref.eval_video("non_finite", "nan_middle")       # NaN in column 3 of rows 7 and 290
    assert np.flatnonzero(np.isnan(z[:, 3])).tolist() == [7, 290]
    got, ds = _alone(z, chunk=32)
    assert not got[1][:7].isnan().any() and got[1][7:, 3].isnan().all() and not got[1][:, :3].isnan().any()
    assert got[2][7:].isnan().all()                      # a NaN logit makes every probability of its row NaN
    ds.reset([0])
    plain = ref.eval_video("non_finite", "plain")[:10]
    ds.push_rows(torch.tensor(plain).cuda())
    dec, mo, mp = ds.decide()
    assert not mo.isnan().any() and not mp.isnan().any()
    assert _same(mo[0], _f32(ref.track(plain)["mean_outputs"][-1]))
    got, _ = _alone(z, chunk=8, window=5)
    nan_rows = got[1][:, 3].isnan().nonzero().flatten().tolist()
    assert nan_rows == list(range(7, 12)) + list(range(290, 295))       # gone once the row has left the window
    assert got[2].isnan().any(dim=1).nonzero().flatten().tolist() == nan_rows


# ---------------------------------------------------------------------------------------------- 6. reset
@pytest.mark.parametrize("window", [None, 5])
def test_reset_in_the_middle_of_a_ragged_schedule_equals_a_fresh_stream(window):
    seqs = list(ref.stream_sequences()[:3])
    ticks = ref.ragged_schedule([len(z) for z in seqs], 8, seed=5)
    cut = next(i for i in range(len(ticks)) if sum(t[1] for t in ticks[:i]) >= 37)
    ds = _cls()(ref.STREAM_C, 3, max_new=8, window=window)
    head, fed = _run(ds, seqs, ticks[:cut])
    t1 = fed[1]
    ds.reset([1])
    assert ds.frames_seen == [fed[0], 0, fed[2]]
    assert ds.decide()[0].cpu()[:, 0].tolist()[1] == -1 and ds.decide()[1][1].isnan().all()
    tail, fed = _run(ds, seqs, ticks[cut:], fed)
    assert ds.frames_seen == [len(seqs[0]), len(seqs[1]) - t1, len(seqs[2])]
    for s in (0, 2):                                                      # untouched, bit for bit
        want, _ = _whole(s, window)
        assert _equal_tracks(tuple(torch.cat([a, b]) for a, b in zip(head[s], tail[s])), want), s
    fresh, _ = _alone(seqs[1][t1:], chunk=8, window=window)
    assert _equal_tracks(tail[1], fresh)
    history, _ = _whole(1, window)
    assert not _same(tail[1][1], history[1][t1:])                         # the history did matter


# ---------------------------------------------------------------------------------------------- 7. wrong tables
def _arena(dtype, shapes, guard, fill):
    """Tensors of ``shapes`` carved out of one allocation, each between slabs of 64 ``guard`` values.  Returns (tensors,
    check): check() is True while every slab is intact."""
    sizes = [int(np.prod(s)) for s in shapes]
    sizes = [(n + 1) & ~1 for n in sizes]                                 # keep every tensor 8-byte aligned
    buf = torch.full((64 + sum(n + 64 for n in sizes),), guard, dtype=dtype, device="cuda")
    out, guards, at = [], [slice(0, 64)], 64
    for shape, n in zip(shapes, sizes):
        t = buf[at:at + int(np.prod(shape))].view(shape)
        t.fill_(fill)
        out.append(t)
        guards.append(slice(at + int(np.prod(shape)), at + n + 64))
        at += n + 64

    def intact():
        parts = torch.cat([buf[g] for g in guards])
        return bool(parts.isnan().all()) if guard != guard else bool((parts == guard).all())
    return out, intact


@pytest.mark.parametrize("window", [None, 5])
def test_a_wrong_table_stays_inside_the_state(window):
    """Stream indices -7 and S + 100, counts above max_count and below 0, offsets before 0 and past M, any position and any
    frame count: the kernel clamps, cuts, masks and bounds, so the launch is in bounds by construction.  It returns, and the
    guard slabs around the state, the rows and the outputs are intact."""
    from feature_vs_text_compound_emotion_amd import ops
    s, c, m, max_count = 3, 7, 11, 4
    (rows, zring), f32_ok = _arena(torch.float32, [(m, c), (s, 16, c)], float("nan"), 0.5)
    (slog, sprob), f64_ok = _arena(torch.float64, [(s, c), (s, c)], float("nan"), 0.0)
    (votes, first), i64_ok = _arena(torch.int64, [(s, c), (s, c)], -12345, 0)
    first.fill_(ops.DECISION_NEVER)
    state = {"zring": zring} if window else {"votes": votes, "first": first, "slog": slog, "sprob": sprob}
    big = 2 ** 31 - 1
    table = torch.tensor([[-7, s + 100, 1, -2 ** 31, big, 0],              # stream
                          [3, 9, 4, big, -5, 2],                           # count
                          [0, m - 1, m + 50, -3, big, 5],                  # offset
                          [2 ** 30 - 1, 0, 123456789, -1, big, 7],         # position
                          [0, -1, 5, big, -2 ** 31, 1],                    # frames, low word
                          [0, -1, 0, big, -2 ** 31, 0]],                   # frames, high word
                         dtype=torch.int32, device="cuda")
    dec, means = ops.decision_stream_push(rows, table, max_count, state, window=window, track=True)
    rdec, rmeans = ops.decision_stream_read(table[:, :s].contiguous(), max_count, state, window=window)
    torch.cuda.synchronize()
    assert f32_ok() and f64_ok() and i64_ok()
    assert dec.shape == (m, 3) and means.shape == (m, 2, c) and rdec.shape == (s, 3) and rmeans.shape == (s, 2, c)
    if window:
        assert torch.isfinite(zring).all()
    else:
        assert int(votes.sum()) > 0 and bool((votes >= 0).all())          # the pushes did land, in some stream's accumulators


# ---------------------------------------------------------------------------------------------- 8. regression
@pytest.mark.parametrize("window", [None, 5])
def test_regression_keeps_the_running_means_only(window):
    rng = np.random.default_rng(9)
    seqs = [np.tanh(rng.standard_normal((90, 2))).astype(np.float32) for _ in range(3)]
    ds = _cls()(2, 3, max_new=8, window=window, task="REGRESSION")
    tracks, _ = _run(ds, seqs, ref.ragged_schedule([90] * 3, 8, seed=2))
    final = ds.decide()
    assert final[0] is None and final[2] is None
    for s in range(3):
        dec, mo, mp = tracks[s]
        assert dec is None and mp is None
        want = _f32(ref.means_only(seqs[s], window=window))
        assert torch.equal(mo, want), s
        assert torch.equal(final[1][s].cpu(), want[-1])
    assert "votes" not in ds.state and "sprob" not in ds.state


# ---------------------------------------------------------------------------------------------- 9. the session
@pytest.mark.parametrize("window", [None, 4])
def test_a_session_feeds_its_decisions_every_row_it_emits(window):
    import test_live_gpu as live_t
    from feature_vs_text_compound_emotion_amd import live
    L, kind = 6, "logmel"
    model = live_t._model(kind)
    raws, pcms = [live_t._raw(L, 1), live_t._raw(L, 2)], [live_t._pcm(0.3, 81), live_t._pcm(0.3, 82)]
    ticks = live_t._ticks([L, L], [pcms[0].shape[0]] * 2, seed=1)
    kw = dict(hold=6, lead=4, max_new=2, max_samples=1024)
    plain = live_t._drive(live.AVStream(model, 2, live_t.FPS, **kw), raws, pcms, ticks, [None])
    sess = live.AVStream(model, 2, live_t.FPS, decisions={"window": window}, **kw)
    assert sess.decisions.max_new == 2 and sess.decisions.n_out == live_t.NCLS
    got = live_t._drive(sess, raws, pcms, ticks, [None])
    assert all(torch.equal(a, b) for a, b in zip(got, plain))            # the session returns what it returned before
    assert sess.frames_seen == [0, 0] and sess.decisions.frames_seen == [L, L]      # finish leaves the decisions to be read
    mine = sess.decisions.decide()
    alone = _cls()(live_t.NCLS, 2, window=window)
    alone.push_ragged(torch.cat(got), [L, L])
    assert all(_same(a, b) for a, b in zip(mine, alone.decide()))
    # the vote against the offline accumulator on stream_forward's logits of the offline-prepared clip
    offline = live_t._reference(kind, L)
    assert torch.equal(torch.stack(got), offline)
    tail = offline if window is None else offline[:, L - window:]
    data = {f"v{i}": {"logits": tail[i].cpu().numpy(), "labels": np.zeros(tail.shape[1], dtype=np.int64)} for i in range(2)}
    assert torch.equal(mine[0][:, 0].cpu(), _offline(data, live_t.NCLS, None)[:, 0])
    # a stream that starts again forgets the finished clip; reset forgets at once
    sess.push(raws[0][:1], [1, 0], pcms[0][:1024], [1024, 0])
    assert sess.decisions.frames_seen == [L, L]                          # nothing emitted yet: the finished clip still stands
    logits, counts = sess.finish([0])
    assert counts == [1, 0] and sess.decisions.frames_seen == [1, L]
    sess.reset()
    assert sess.decisions.frames_seen == [0, 0] and sess.decisions.decide()[0].cpu().tolist() == [[-1] * 3] * 2
    with pytest.raises(ValueError, match="max_new"):
        live.AVStream(model, 2, live_t.FPS, decisions={"max_new": 1}, **kw)
    with pytest.raises(ValueError, match="task"):
        live.AVStream(model, 2, live_t.FPS, decisions={"task": "REGRESSION"}, **kw)
    with pytest.raises(ValueError, match="window"):
        live.AVStream(model, 2, live_t.FPS, decisions={"window": 0}, **kw)
