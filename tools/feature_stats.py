"""Per-component mean and std of the ``vggish`` and ``bert`` rows the fused extractor makes of a trial list -> the pickle that
``MultimodalFeatureExtractor(mean_std=)``, ``AVStream(mean_std=)`` and ``TrialDataset(mean_std=)`` take (the reference's
``mean_std_info_fold-{j}.pkl``, base/experiment.py:242-269).

    python tools/feature_stats.py --trials trials.txt --out mean_std_info_fold-0.pkl [--fps 30] [--features vggish bert]
                                  [--sample-rate 16000 --resample kaiser_best] [--audio-state vggish.pt] [--bert-state bert.pt]

``trials.txt`` names one trial directory per line (train + valid, as the reference merges them), optionally followed by a
comma and the trial's number of frames.  A trial directory holds

    pcm.npy              int16 [S] or [S, channels]: the trial's whole audio track
    token_ids.npy        int64 [N, T]: the transcript's N sentences, each [CLS] .. [SEP] padded with 0 to T tokens
    attention_mask.npy   int64 [N, T]
    video.npy            only its first dimension is read (memory-mapped), when the list gives no frame count

Every trial is taken once and whole, over its true frames with no window padding, as the reference's ``calc_mean_std_fn`` does
with ``windowing=False``: the extractor runs on the trial, its rows feed a ``FeatureMoments`` (float64 sums on the device, one
launch per call, no host synchronisation), and the statistics are finalised on the host by the reference's formulas.  Under
``torchrun`` the trials are dealt to the ranks in turn and the sums are all-reduced; rank 0 writes the file.  ``logmel`` and
``video`` have no statistics: the reference wraps neither in ``Normalize``.  Needs the GPU.
"""
import argparse
import os
import sys

sys.modules.setdefault("triton", None)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def read_trials(path):
    """-> [(directory, frames or None)]; relative directories are taken from the list's own."""
    trials, base = [], os.path.dirname(os.path.abspath(path))
    with open(path) as fh:
        for line in fh:
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            name, _, frames = line.partition(",")
            trials.append((os.path.join(base, name.strip()), int(frames) if frames.strip() else None))
    if not trials:
        raise SystemExit(f"{path}: no trial")
    return trials


def trial_rows(extractor, directory, frames, features, sample_rate=16000, resample=None, device="cuda"):
    """{feature: [frames, C] device rows} of one trial, raw (the extractor must not standardise)."""
    if extractor.standardizer is not None:
        raise ValueError("feature statistics are those of the raw rows: build the extractor without mean_std")
    if frames is None:
        frames = int(np.load(os.path.join(directory, "video.npy"), mmap_mode="r").shape[0])
    if frames < 1:
        raise ValueError(f"{directory}: {frames} frames")
    rows = {}
    if "vggish" in features:
        pcm = torch.from_numpy(np.ascontiguousarray(np.load(os.path.join(directory, "pcm.npy")))).to(device)
        rows["vggish"] = extractor.audio_features(pcm[None], frames, sample_rate, resample)[0, 0]
    if "bert" in features:
        ids = torch.from_numpy(np.load(os.path.join(directory, "token_ids.npy")).astype(np.int64))
        mask = torch.from_numpy(np.load(os.path.join(directory, "attention_mask.npy")).astype(np.int64))
        rows["bert"] = extractor.paragraph_features(ids.to(device), mask.to(device), [ids.shape[0]], frames,
                                                    attention_mask_cpu=mask)[0, 0]
    return rows


def collect(extractor, trials, features, sample_rate=16000, resample=None, device="cuda", rank=0, world=1):
    """A ``FeatureMoments`` over this rank's share of ``trials``."""
    from feature_vs_text_compound_emotion_amd.feature_stats import FeatureMoments
    dims = {"vggish": 128, "bert": extractor.text.hidden}
    acc = FeatureMoments({f: dims[f] for f in features}, device)
    for directory, frames in trials[rank::world]:
        for f, r in trial_rows(extractor, directory, frames, features, sample_rate, resample, device).items():
            acc.update(f, r)
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--fps", type=float, default=30.0)
    ap.add_argument("--features", nargs="+", default=["vggish", "bert"], choices=["vggish", "bert"])
    ap.add_argument("--sample-rate", type=int, default=16000)
    ap.add_argument("--resample", default=None, choices=["kaiser_best", "kaiser_fast"])
    ap.add_argument("--audio-state", default=None, help="state dict of the VGGish backbone (torch.save)")
    ap.add_argument("--bert-state", default=None, help="state dict of the BERT encoder (torch.save)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("feature_stats.py runs the extractor on the GPU; none is visible")
    from feature_vs_text_compound_emotion_amd.feature_extractor import MultimodalFeatureExtractor
    from feature_vs_text_compound_emotion_amd.feature_stats import save_mean_std
    rank, world = 0, int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        from feature_vs_text_compound_emotion_amd.data_parallel import init_process_group_from_env
        rank, world, _ = init_process_group_from_env()
    fx = MultimodalFeatureExtractor(fps=a.fps)
    if a.audio_state:
        fx.audio.backbone.load_state_dict(torch.load(a.audio_state, map_location="cpu"))
    if a.bert_state:
        fx.text.load_state_dict(torch.load(a.bert_state, map_location="cpu"))
    fx = fx.cuda().eval()
    acc = collect(fx, read_trials(a.trials), a.features, a.sample_rate, a.resample, "cuda", rank, world)
    if world > 1:
        acc.all_reduce()
    if rank == 0:
        save_mean_std(a.out, acc.finalize())
        print({f: n for f, n in acc.count.items()}, "->", a.out)


if __name__ == "__main__":
    main()
