"""What scoring a conversion by its PPG round trip adds (Synthesizer.convert_scored against Synthesizer.convert), and the DTW alone.

Default: the 16 ragged 1 - 4 s wavs, models and seeds of tools/time_wav2wav.py --shape ragged (synthetic nnet3 TDNN, senone
PPG -> mel model, hop-256 vocoder, stop gate closed).  ``convert`` and ``convert_scored`` alternate in ONE process, the host
clock around each call (wav objects in, samples on the host out, synchronised), --reps calls of each after a warm-up; then the two
parts of what scoring adds, each alone and synchronised: the front-end pass over the 2 B utterances (ppg.compute_ppg_padded,
monophone classes; convert's own pass over B senone utterances is reported next to it) and facppg.score.ppg_dtw over its rows.
--root DIR imports the package from another checkout; one without facppg.score (the parent commit) reports ``convert`` alone.

--dtw: no models -- facppg.score.ppg_dtw alone on B = 16 pairs of Ta = Tb = 600 frames, D = 40 random posteriors, band 0 and 60,
three warm-up and --reps timed calls per band (host clock, synchronised).  Under ``rocprofv3 --kernel-trace --stats`` this is the
run the per-kernel times come from: every call launches k_dtw_prep twice, k_dtw_dist and k_dtw_sweep once.

Prints one JSON line; --out FILE appends it there.

  python tools/time_roundtrip.py [--reps 8] [--root DIR] [--out FILE]
  python tools/time_roundtrip.py --dtw [--reps 5] [--out FILE]
"""
import argparse
import contextlib
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


def emit(res, out):
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtw", action="store_true")
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

    if args.dtw:
        from facppg import score
        B, T, D = 16, 600, 40
        gen = torch.Generator(device="cuda").manual_seed(args.seed)
        a = torch.softmax(3.0 * torch.randn(B, D, T, device="cuda", generator=gen), dim=1)
        b = torch.softmax(torch.log(a + 1e-12) + 0.7 * torch.randn(B, D, T, device="cuda", generator=gen), dim=1)
        res = {"workload": "facppg.score.ppg_dtw alone: B = %d pairs, Ta = Tb = %d, D = %d" % (B, T, D), "device": torch.cuda.get_device_name(0),
               "reps": args.reps}
        for band in (0, 60):
            for _ in range(3):
                _, out = timed(lambda: score.ppg_dtw(a, [T] * B, b, [T] * B, band=band))
            res["band_%d" % band] = dict(stats([timed(lambda: score.ppg_dtw(a, [T] * B, b, [T] * B, band=band))[0] for _ in range(args.reps)]),
                                         mean_distance=float(out["distance"].mean()), mean_steps=float(out["steps"].mean()))
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
    scored = hasattr(s, "convert_scored")

    def plain():
        return s.convert(wavs, deps, **kw)

    def with_scores():
        return s.convert_scored(wavs, deps, **kw)

    for _ in range(3):
        _, (audio, tout) = timed(plain)
        if scored:
            _, (audio_s, tout_s, scores) = timed(with_scores)
    assert tout == frames and all(np.isfinite(w).all() and w.shape == (256 * n,) for w, n in zip(audio, frames))
    t_plain, t_scored = [], []
    for _ in range(args.reps):
        t_plain.append(timed(plain)[0])
        if scored:
            t_scored.append(timed(with_scores)[0])
    res = {"workload": "wav -> wav, 16 utterances, %d frames (%.1f s of audio), TDNN hidden %d, 5816 senones, hop 256" % (
               sum(frames), sum(frames) / 100.0, args.hidden),
           "root": os.path.basename(root), "device": torch.cuda.get_device_name(0), "reps": args.reps, "convert": stats(t_plain)}
    if scored:
        from facppg import score
        assert all(np.array_equal(x, y) for x, y in zip(audio, audio_s)) and tout_s == tout
        back = [feat.WaveData(16000.0, torch.from_numpy(w).cuda()[None] * 32768.0) for w in audio]

        def front2():
            return ppg.compute_ppg_padded(wavs + back, deps, is_full_ppg=False)

        def front1():
            return ppg.compute_ppg_padded(wavs, deps, is_full_ppg=True)
        for _ in range(3):
            _, (x, fr) = timed(front2)
            timed(front1)
        B = len(wavs)

        def dtw():
            return score.ppg_dtw(x[:B], fr[:B], x[B:], fr[B:])
        for _ in range(3):
            timed(dtw)
        res.update({"convert_scored": stats(t_scored),
                    "added_ms": statistics.median(t_scored) - statistics.median(t_plain),
                    "front_end_2B_monophone_alone": stats([timed(front2)[0] for _ in range(args.reps)]),
                    "front_end_B_senone_alone": stats([timed(front1)[0] for _ in range(args.reps)]),
                    "ppg_dtw_alone": stats([timed(dtw)[0] for _ in range(args.reps)]),
                    "teacher_frames": scores["teacher_frames"].tolist(), "roundtrip_frames": scores["roundtrip_frames"].tolist(),
                    "mean_distance": float(scores["distance"].mean()), "mean_agreement": float(scores["agreement"].mean()),
                    "mean_stretch": float(scores["stretch"].mean())})
    emit(res, args.out)


if __name__ == "__main__":
    main()
