"""What the per-phone report adds to a scored conversion (Synthesizer.convert_scored(phones=True) against convert_scored()), and the
aligner's three kernels alone.

Default: the 16 ragged 1 - 4 s wavs, models and seeds of tools/time_wav2wav.py --shape ragged (synthetic nnet3 TDNN, senone
PPG -> mel model, hop-256 vocoder, stop gate closed), as tools/time_roundtrip.py times them.  ``convert_scored()`` and
``convert_scored(phones=True)`` alternate in ONE process, the host clock around each call (wav objects in, samples on the host
out, synchronised), --reps calls of each after a warm-up; then facppg.align.phone_report alone over the round trip's padded batch,
synchronised.  --root DIR imports the package from another checkout; one whose convert_scored has no ``phones`` (the parent
commit) reports ``convert_scored`` alone.  The synthetic acoustic model's posteriors have one class on top almost everywhere, so
the teachers decode to a handful of phones: this run times the report's launches, copies and host work, not long sequences.

--kernels: no models -- emissions, decode and forced alignment on B = 16 utterances of T = 600 frames, D = 40 posteriors that HAVE
phones (runs of 1 - 12 frames of a random class, +4 on the run's logit: about 90 runs per utterance; the last class is the
optional ``sil``), the "conversion" a second draw over the same runs: facppg.align.phone_report, three warm-up and --reps timed
calls (host clock, synchronised).  Under ``rocprofv3 --kernel-trace --stats`` this is the run the per-kernel times come from: every
call launches k_align_emit twice, k_align_decode and k_align_force once.

Prints one JSON line; --out FILE appends it there.

  python tools/time_align.py [--reps 8] [--root DIR] [--out FILE]
  python tools/time_align.py --kernels [--reps 10] [--out FILE]
"""
import argparse
import contextlib
import inspect
import io
import json
import os
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def synthetic_wav(np, n, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n) / 16000.0
    x = 6000 * np.sin(2 * np.pi * 220 * t) + 2500 * np.sin(2 * np.pi * 1370 * t + 1.0) + 300 * g.standard_normal(n)
    return np.round(x).astype(np.int16)


def phone_posteriors(np, B, T, D, seed):
    """Two draws [B, D, T] over the same runs of 1 - 12 frames of a random class: softmax of randn with +4 on the run's class."""
    g = np.random.Generator(np.random.PCG64(seed))
    hot = np.zeros((B, T), dtype=np.int64)
    for b in range(B):
        t = 0
        while t < T:
            n, k = int(g.integers(1, 13)), int(g.integers(D))
            hot[b, t:t + n] = k
            t += n
    out = []
    for _ in range(2):
        z = g.standard_normal((B, D, T))
        np.put_along_axis(z, hot[:, None, :], np.take_along_axis(z, hot[:, None, :], 1) + 4.0, 1)
        p = np.exp(z - z.max(axis=1, keepdims=True))
        out.append((p / p.sum(axis=1, keepdims=True)).astype(np.float32))
    return out


def emit(res, out):
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--out")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path[:0] = [root, os.path.join(root, "fac-via-ppg_amd")]
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path"

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    if args.kernels:
        from facppg import align
        B, T, D = 16, 600, 40
        a, b = (torch.from_numpy(v).cuda() for v in phone_posteriors(np, B, T, D, args.seed))

        def report():
            return align.phone_report(a, [T] * B, b, [T] * B)
        for _ in range(3):
            _, (reports, kept) = timed(report)
        res = {"workload": "facppg.align.phone_report alone: B = %d utterances, T = %d, D = %d" % (B, T, D), "device": torch.cuda.get_device_name(0),
               "reps": args.reps, "phone_report": stats([timed(report)[0] for _ in range(args.reps)]),
               "states": [len(r) for r in reports], "mean_phones_kept": float(kept.mean())}
        emit(res, args.out)
        return

    from scipy.io import wavfile
    import ppg
    from common import feat, nnet3
    from common.hparams import create_hparams_stage
    from facppg import pipeline, synth
    from script.train_ppg2mel import load_model
    from waveglow.denoiser import Denoiser
    from waveglow.glow import WaveGlow
    kf = os.path.join(root, "tests", "golden", "kaldi_feats")
    g = np.random.Generator(np.random.PCG64(args.seed))
    frames = (100 + g.integers(0, 301, size=16)).tolist()
    tmp = tempfile.TemporaryDirectory()
    net = nnet3.synthetic_tdnn(input_dim=40, hidden=args.hidden, output_dim=5816, norm="renorm", seed=3, lda=False)
    nnet3.write_nnet3(os.path.join(tmp.name, "final.raw"), net)
    deps = ppg.DependenciesPPG(nnet_path=os.path.join(tmp.name, "final.raw"), lda_path=os.path.join(kf, "final.mat"),
                               reduce_dim_path=os.path.join(kf, "reduce_dim.mat"), splice_opts_path=os.path.join(kf, "splice_opts"))
    paths = []
    for i, n in enumerate(frames):
        paths.append(os.path.join(tmp.name, "utt%02d.wav" % i))
        wavfile.write(paths[-1], 16000, synthetic_wav(np, 160 * n, 900 + i))
    cfg = dict(synth.WAVEGLOW_CONFIG, hop_length=256)
    wg = WaveGlow.remove_weightnorm(WaveGlow(**cfg))
    wg.load_state_dict(synth.waveglow_state_dict(cfg))
    wg = wg.cuda().eval()
    hp = create_hparams_stage(max_decoder_steps=max(frames))
    with contextlib.redirect_stdout(io.StringIO()):
        taco = load_model(hp)
    taco.load_state_dict(synth.tacotron_state_dict(hp, gate_bias=-10.0))
    taco.eval()
    s = pipeline.Synthesizer.__new__(pipeline.Synthesizer)        # (the models of the tests: no checkpoint files)
    s.hparams, s.tacotron, s.waveglow, s.denoiser = hp, taco, wg, Denoiser(wg, hop_length=256, mode="zeros")
    s.vocoder_arithmetic = s.vocoder_stream = None
    kw = dict(utterance_seeds=[11 + 2 * i for i in range(len(frames))], step_limits=list(frames))
    wavs = [feat.read_wav_kaldi(p) for p in paths]
    has_phones = "phones" in inspect.signature(s.convert_scored).parameters

    def scored():
        return s.convert_scored(wavs, deps, **kw)

    def with_phones():
        return s.convert_scored(wavs, deps, phones=True, **kw)

    for _ in range(3):
        _, (audio, tout, scores) = timed(scored)
        if has_phones:
            _, (audio_p, tout_p, scores_p) = timed(with_phones)
    assert tout == frames and all(np.isfinite(w).all() and w.shape == (256 * n,) for w, n in zip(audio, frames))
    t_scored, t_phones = [], []
    for _ in range(args.reps):
        t_scored.append(timed(scored)[0])
        if has_phones:
            t_phones.append(timed(with_phones)[0])
    res = {"workload": "wav -> wav, 16 utterances, %d frames (%.1f s of audio), TDNN hidden %d, 5816 senones, hop 256" % (
               sum(frames), sum(frames) / 100.0, args.hidden),
           "root": os.path.basename(root), "device": torch.cuda.get_device_name(0), "reps": args.reps, "convert_scored": stats(t_scored)}
    if has_phones:
        from facppg import align
        assert all(np.array_equal(x, y) for x, y in zip(audio, audio_p)) and tout_p == tout
        assert all(scores[k].tobytes() == scores_p[k].tobytes() for k in scores)
        back = [feat.WaveData(16000.0, torch.from_numpy(w).cuda()[None] * 32768.0) for w in audio]
        x, fr = ppg.compute_ppg_padded(wavs + back, deps, is_full_ppg=False)
        B = len(wavs)

        def report():
            return align.phone_report(x[:B], fr[:B], x[B:], fr[B:])
        for _ in range(3):
            timed(report)
        res.update({"convert_scored_phones": stats(t_phones), "added_ms": statistics.median(t_phones) - statistics.median(t_scored),
                    "phone_report_alone": stats([timed(report)[0] for _ in range(args.reps)]),
                    "states": [len(r) for r in scores_p["phones"]], "mean_phones_kept": float(scores_p["phones_kept"].mean()),
                    "teacher_frames": scores["teacher_frames"].tolist(), "roundtrip_frames": scores["roundtrip_frames"].tolist()})
    emit(res, args.out)


if __name__ == "__main__":
    main()
