"""The resampling front end without a GPU: the float64 restatement (tests/resample_ref.py) against analytic tones, the
package's polyphase tap table against that restatement, and the host-side rules (output length, table cap, refusals)."""
import math

import numpy as np
import pytest

import resample_ref as R

RATES = (48000, 44100, 22050, 8000)
FILTERS = ("kaiser_best", "kaiser_fast")


@pytest.mark.parametrize("filter,bar", [("kaiser_best", 1e-7), ("kaiser_fast", 1e-4)])
@pytest.mark.parametrize("sr", RATES)
def test_reference_resamples_tones_below_the_passband_edge(sr, filter, bar):
    """Checks the DEFINITION without resampy: eight tones between 50 Hz and 0.8 x rolloff x min(sr, 16000) / 2 of
    amplitude 0.02 .. 0.1, 0.25 s long, resampled, against the same tones evaluated at n / 16000; the outputs within the
    filter's reach of either end (where the sum is cut short) are skipped.  The bars, 1e-7 and 1e-4, are about 5 x
    the worst seen over tone draws (1.4e-8 for kaiser_best, 2.1e-5 for kaiser_fast; this draw: 1.1e-8 and 1.5e-5)."""
    zeros, _, rolloff = R.FILTERS[filter]
    rng = np.random.default_rng(20240)
    freqs = rng.uniform(50.0, 0.8 * rolloff * min(sr, 16000) / 2.0, 8)
    amps = rng.uniform(0.02, 0.1, 8)
    phases = rng.uniform(0.0, 2.0 * np.pi, 8)

    def tones(t):
        return (amps[:, None] * np.sin(2.0 * np.pi * freqs[:, None] * t[None, :] + phases[:, None])).sum(0)
    x = tones(np.arange(int(0.25 * sr)) / float(sr))
    y = R.resample_ref(x, sr, filter)
    ratio = 16000.0 / sr
    assert y.shape == (int(len(x) * ratio),)
    skip = int(math.ceil(zeros / min(1.0, ratio) * ratio)) + 2
    want = tones(np.arange(len(y)) / 16000.0)
    err = np.abs(y - want)[skip:len(y) - skip].max()
    print(f"\n[tones {sr} {filter}] {len(y) - 2 * skip} outputs compared, max err {err:.2e}", end="")
    assert len(y) > 2 * skip + 100 and err < bar


@pytest.mark.parametrize("filter", FILTERS)
@pytest.mark.parametrize("sr", RATES)
def test_tap_table_equals_the_direct_form(sr, filter):
    """Bar 1e-12: at most T <= 772 products of magnitude <= 1 per output, each side rounding at 1.1e-16."""
    from feature_vs_text_compound_emotion_amd.audio_backbone import resample_taps, resampled_length
    taps, L, M = resample_taps(sr, filter)
    g = math.gcd(16000, sr)
    zeros = R.FILTERS[filter][0]
    J = int(math.ceil(zeros / min(1.0, 16000.0 / sr)))
    assert (L, M) == (16000 // g, sr // g) and taps.shape == (L, 2 * J + 2) and taps.dtype == np.float64
    assert taps.shape[1] <= 772
    x = np.random.default_rng(sr).uniform(-1.0, 1.0, (2, 1500))
    n_out = resampled_length(x.shape[1], sr)
    err = np.abs(R.apply_taps(x, taps, L, M, n_out) - R.resample_ref(x, sr, filter)).max()
    print(f"\n[table {sr} {filter}] {L} x {taps.shape[1]} taps, {n_out} outputs, max err {err:.2e}", end="")
    assert err < 1e-12


def test_tap_table_at_16_khz_is_the_identity():
    from feature_vs_text_compound_emotion_amd.audio_backbone import resample_taps
    taps, L, M = resample_taps(16000, "kaiser_best")
    assert (L, M) == (1, 1) and taps.tolist() == [[1.0, 0.0]]


@pytest.mark.parametrize("sr", RATES + (16000, 11025, 96000))
def test_output_length_is_the_python_float_expression(sr):
    from feature_vs_text_compound_emotion_amd.audio_backbone import resampled_length
    for n_in in (16001, 44100 + 441, 96000, 7):
        assert resampled_length(n_in, sr) == int(n_in * (16000.0 / sr))


def test_refusals_happen_on_the_host():
    from feature_vs_text_compound_emotion_amd.audio_backbone import MAX_RESAMPLE_TAPS, VGGish, resample_taps
    assert MAX_RESAMPLE_TAPS == 1 << 22
    assert resample_taps(44100, "kaiser_best")[0].shape == (160, 356)           # the largest table of the usual rates
    with pytest.raises(ValueError, match="tap table"):
        resample_taps(44101, "kaiser_best")                                     # 16000 x 356 entries
    resample_taps(16001, "kaiser_best")                                         # 16000 x 132: under the cap
    with pytest.raises(ValueError, match="unknown resampling filter"):
        resample_taps(44100, "sinc_best")
    for bad in (0, -8000, 22050.5):
        with pytest.raises(ValueError):
            resample_taps(bad, "kaiser_fast")
    net = VGGish()      # on the CPU: every refusal below comes before the module touches a device
    pcm = np.zeros(44100, dtype=np.int16)
    with pytest.raises(ValueError, match="resample="):
        net.wav_int16_to_examples(pcm, 44100)
    with pytest.raises(ValueError, match="resample="):
        net.wav_int16_to_examples(pcm, 44100, 0.96, 0.96, resample=None)
    with pytest.raises(ValueError, match="unknown resampling filter"):
        net.wav_int16_to_examples(pcm, 44100, resample="sinc_best")
    with pytest.raises(ValueError, match="positive integer"):
        net.wav_int16_to_examples(pcm, 0, resample="kaiser_best")
