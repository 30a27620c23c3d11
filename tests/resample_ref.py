"""The resampling front end restated in numpy float64, for ``tests/test_resample_cpu.py`` and ``tests/test_resample_gpu.py``.

The definition (band-limited sinc interpolation as ``resampy.resample`` states it, with the window evaluated where it
is needed instead of looked up in a sampled table), for ``ratio = 16000 / sr_in`` and ``scale = min(1, ratio)``:

  y[n] = scale * sum_k x[k] * h(scale * (n / ratio - k)),   k over the valid input indices,   n < int(len(x) * ratio)
  h(u) = rolloff * sinc(rolloff * u) * I0(beta * sqrt(1 - (u / zeros)^2)) / I0(beta)   for |u| < zeros, else 0

``resample_ref`` is the direct form: one loop over the outputs, ``scipy.special.i0``, no table, no phases.  The only
liberty it takes is to write ``n / ratio - k`` as ``(n * M - k * L) / L`` with ``L / M = ratio`` in lowest terms: the
numerator is an exact integer, so the argument of ``h`` carries ONE rounding (relative 1.1e-16) instead of the absolute
3.6e-12 that ``n / ratio`` near 3e4 would lose before the subtraction.  That is what lets the 1e-12 bars of the tests
stand on summation error alone.

The filter constants are restated here, not imported from the package.
"""
import math

import numpy as np
from scipy.special import i0

SAMPLE_RATE = 16000
FILTERS = {"kaiser_best": (64, 14.769656459379492, 0.9475937167399596), "kaiser_fast": (16, 8.555504641634386, 0.85)}


def kaiser_sinc(u, filter):
    zeros, beta, rolloff = FILTERS[filter]
    u = np.asarray(u, dtype=np.float64)
    inside = np.abs(u) < zeros
    win = i0(beta * np.sqrt(np.where(inside, 1.0 - (u / zeros) ** 2, 0.0))) / i0(beta)
    return np.where(inside, rolloff * np.sinc(rolloff * u) * win, 0.0)


def resample_ref(x, sr_in, filter):
    """x [..., N] float64 at ``sr_in`` -> [..., int(N * (16000.0 / sr_in))] at 16 kHz.  At 16 kHz: x itself, as the
    reference does not call the resampler then (vggish_input.py:55)."""
    x = np.asarray(x, dtype=np.float64)
    if sr_in == SAMPLE_RATE:
        return x.copy()
    zeros = FILTERS[filter][0]
    n_in = x.shape[-1]
    ratio = float(SAMPLE_RATE) / sr_in
    scale = min(1.0, ratio)
    g = math.gcd(SAMPLE_RATE, sr_in)
    L, M = SAMPLE_RATE // g, sr_in // g
    reach = int(math.ceil(zeros / scale)) + 1     # h is zero beyond: the sum over all k, without the zero terms
    y = np.zeros(x.shape[:-1] + (int(n_in * ratio),))
    for n in range(y.shape[-1]):
        centre = (n * M) // L
        k = np.arange(max(0, centre - reach), min(n_in, centre + reach + 1))
        y[..., n] = scale * (x[..., k] @ kaiser_sinc(scale * ((n * M - k * L) / float(L)), filter))
    return y


def mixdown_pad_ref(pcm_int16, channels, pad):
    """int16 [clips, S] (channels == 1) or interleaved [clips, S, C] -> float64 [clips, S + pad]: / 32768, mean over the
    channels, ``pad`` samples of edge padding (vggish_input.py:95, :51-53, :97 in the order the front end applies them)."""
    x = np.asarray(pcm_int16).astype(np.float64) / 32768.0
    if channels > 1 or x.ndim == 3:
        assert x.shape[-1] == channels
        x = np.mean(x, axis=-1)
    return np.pad(x, [(0, 0)] * (x.ndim - 1) + [(0, pad)], "edge")


def apply_taps(x, taps, L, M, n_out):
    """The polyphase form the kernel computes, in numpy: out[n] = sum_j taps[r][j] * x[q - J + j], zeros outside x;
    q, r = divmod(n M, L), J = (T - 2) / 2.  For n_out <= int(len(x) * L / M)."""
    T = taps.shape[1]
    J = (T - 2) // 2
    xz = np.concatenate([np.zeros(x.shape[:-1] + (J,)), x, np.zeros(x.shape[:-1] + (T + 1,))], axis=-1)
    y = np.zeros(x.shape[:-1] + (n_out,))
    for n in range(n_out):
        q, r = divmod(n * M, L)
        y[..., n] = xz[..., q:q + T] @ taps[r]     # q < len(x) for n < int(len(x) * L / M): inside the zero margin
    return y


def wav_to_examples_ref(pcm, sr, channels, filter, window_sec, hop_sec):
    """int16 [S] (``channels`` == 1) or [S, C] at ``sr`` -> the reference's examples [n, 96, 64] float64: mix, pad one
    second at the input rate, resample, then the oracle's 16 kHz ``waveform_to_examples``.  With one more leading axis:
    clips of one length, resampled in one pass of the loop -> [clips, n, 96, 64]."""
    import oracle
    pcm = np.asarray(pcm)
    batched = pcm.ndim == (3 if channels > 1 else 2)
    samples = resample_ref(mixdown_pad_ref(pcm if batched else pcm[None], channels, sr), sr, filter)
    ex = np.stack([oracle.waveform_to_examples(row, SAMPLE_RATE, window_sec, hop_sec) for row in samples])
    return ex if batched else ex[0]
