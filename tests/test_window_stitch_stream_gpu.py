"""``cer_window_stitch_stream`` alone: the frames of live streams stitched from the ring of their last window outputs, against a
numpy float32 mirror of the offline stitch (a sequential sum from 0 in ascending window start, the tail last, one division by
the count).  Every comparison is for equality."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (W, H) -> n of the stream that ended past one wrap of its ring; (8, 3): starts 0, 3, 6, 9 and the tail 11
ENDED = {(8, 3): 19, (4, 4): 22, (4, 1): 11}


def _mirror(wring, hop, rows, done, tail):
    s_, k, w, c = wring.shape
    out = np.zeros((len(rows), c), np.float32)
    for p, (s, f) in enumerate(rows):
        for ch in range(c):
            acc, cnt = np.float32(0.0), 0
            for i in range(max(done[s] - (k - 1), 0), done[s]):
                r = f - i * hop
                if 0 <= r < w:
                    acc = np.float32(acc + wring[s, i % (k - 1), r, ch])
                    cnt += 1
            r = f - tail[s]
            if tail[s] >= 0 and 0 <= r < w:
                acc = np.float32(acc + wring[s, k - 1, r, ch])
                cnt += 1
            assert cnt > 0
            out[p, ch] = acc / np.float32(cnt)
    return out


@pytest.mark.parametrize("c", [1, 7, 8])
@pytest.mark.parametrize("w,h", sorted(ENDED))
def test_three_streams_in_one_launch_equal_the_sequential_sum(w, h, c):
    from feature_vs_text_compound_emotion_amd import ops
    from feature_vs_text_compound_emotion_amd.trainer import windowing
    from feature_vs_text_compound_emotion_amd.window_stream import ring_windows
    k, n, short = ring_windows(w, h), ENDED[(w, h)], w // 2 + 1
    starts = [int(wd[0]) for wd in windowing(np.arange(n), w, h)]
    regular = [s for s in starts if s % h == 0 and s + w <= n]
    has_tail = len(regular) < len(starts)
    assert len(regular) > k - 1 and has_tail == (h > 1)       # past one wrap; a tail whose start is no multiple of H
    if (w, h) == (8, 3):
        assert starts == [0, 3, 6, 9, 11] and short == 5
    # stream 0 ended after n frames; stream 1 ended after ``short`` < W frames; stream 2 is under way and emits nothing
    done, tail = [len(regular), 0, 2], [starts[-1] if has_tail else -1, 0, -1]
    g = torch.Generator().manual_seed(1000 * w + 10 * h + c)
    host = torch.full((3, k, w, c), float("nan"))
    for i in range(max(done[0] - (k - 1), 0), done[0]):                     # the windows stream 0 still holds
        host[0, i % (k - 1)] = torch.randn(w, c, generator=g)
    if has_tail:
        host[0, k - 1] = torch.randn(w, c, generator=g)
    host[1, k - 1, :short] = torch.randn(short, c, generator=g)             # the short window's rows; the rest stays NaN
    # the frames of stream 0 none of whose windows has left the ring
    first = next(f for f in range(n) if max((f - w) // h + 1, 0) >= done[0] - (k - 1))
    rows = [(1, f) for f in range(short)] + [(0, f) for f in range(first, n)]
    # NaN guards around the ring and around the output
    big = torch.full((5, k, w, c), float("nan"), device="cuda")
    big[1:4] = host.cuda()
    buf = torch.full((len(rows) + 2, c), float("nan"), device="cuda")
    got = ops.window_stitch_stream(big[1:4], h, rows, done, tail, out=buf[1:-1])
    assert got.data_ptr() == buf[1].data_ptr()
    want = _mirror(host.numpy(), h, rows, done, tail)
    assert np.isfinite(want).all()
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert torch.isnan(buf[0]).all() and torch.isnan(buf[-1]).all()
    assert torch.isnan(big[0]).all() and torch.isnan(big[4]).all() and torch.isnan(big[3]).all()
    assert torch.equal(torch.isnan(big[1:4]).cpu(), torch.isnan(host))      # the ring is read, never written


def test_the_stitch_equals_the_offline_kernel_on_the_same_windows():
    """Stream 0 of the (8, 3) case: the live stitch of frames 8 .. 18 is the offline ``stitch_windows`` of all five windows."""
    from feature_vs_text_compound_emotion_amd import ops
    from feature_vs_text_compound_emotion_amd.eval_device import stitch_windows
    w, h, n, c, k = 8, 3, 19, 7, 4
    starts = [0, 3, 6, 9, 11]
    wins = torch.randn(5, w, c, generator=torch.Generator().manual_seed(3)).cuda()
    offline = stitch_windows(wins, starts, n)
    ring = torch.zeros((1, k, w, c), device="cuda")
    for i in (1, 2, 3):
        ring[0, i % (k - 1)] = wins[i]
    ring[0, k - 1] = wins[4]
    live = ops.window_stitch_stream(ring, h, [(0, f) for f in range(8, n)], [4], [11])
    assert torch.equal(live, offline[8:])
