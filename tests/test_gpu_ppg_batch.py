"""GPU: the batched wav -> PPG front end (facppg_mfcc_compute_batch, facppg_cmn_splice_transform_batch,
facppg_tdnn_forward_batch[_reduced]; ppg.compute_*_batch, common.data_utils.get_ppg_batch / PPGMelLoader,
script.synthesize_corpus --wav_list) against the NumPy oracles, against itself with other neighbours in the batch, and
against the single-utterance entry points.

The acoustic model is a small synthetic nnet3 TDNN written to a temporary directory, as in test_gpu_tdnn.py: splices
(-2..2), (-1, 2), (-3, 3), (0): two dilated layers, left context 6 != right context 7, renorm layers, a softmax; LDA and
pdf -> monophone map are the reference's own files (tests/golden/kaldi_feats).

Shapes.  Frames (1, 5, 37, 150): shorter than either context, shorter than left + right, no multiple of a column tile,
the size of the existing test.  Their segments take 16 + 20 + 52 + 164 = 252 columns: the 32-column GEMM kernel (up to 256
columns); the batch (150, 150) takes 328 and crosses into the 64-column kernel.  The wav of the 37-frame utterance is
sampled at 44.1 kHz (the downsample branch).

Bounds against the oracle are those of test_gpu_tdnn.py / test_gpu_feat.py.  Against the single-utterance calls: the MFCC,
the CMN / splice / LDA output, and the whole TDNN of a one-utterance batch (same GEMM kernel, sums per column: the renorm
and the softmax then see equal inputs) are equal bit for bit; through the GEMM layers of a wider batch the deviation is held to
twice what two runs of the SAME utterance show between FACPPG_GEMM_SHAPE=legacy and the default (two summation orders of
the existing code; both are reassociations of the same fp32 sums, hence the factor 2), and to 2e-6 in any case."""
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from oracle import feat as of
from oracle import nnet3 as onnet3
from test_feat_cpu import KF, synthetic_wav

pytestmark = pytest.mark.gpu

FRAMES = (1, 5, 37, 150)
WAVS = ((160, 16000), (800, 16000), (16317, 44100), (24000, 16000))      # samples, rate -> FRAMES at a 10 ms shift


def _model(tmp, output):
    from common import decode, nnet3
    net = nnet3.synthetic_tdnn(input_dim=40, hidden=128, output_dim=5816, norm="renorm", output=output, seed=3, lda=False)
    path = str(tmp / ("final_%s.raw" % output))
    nnet3.write_nnet3(path, net)
    return path, decode.read_nnet3_model(path)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The models, the dependencies, the utterances (features and wavs) and their oracle answers, computed once."""
    import ppg
    tmp = tmp_path_factory.mktemp("ppg_batch")
    nnet_path, model = _model(tmp, "softmax")
    _, model_log = _model(tmp, "log-softmax")
    deps = ppg.DependenciesPPG(nnet_path=nnet_path, lda_path=os.path.join(KF, "final.mat"),
                               reduce_dim_path=os.path.join(KF, "reduce_dim.mat"), splice_opts_path=os.path.join(KF, "splice_opts"))
    g = np.random.Generator(np.random.PCG64(21))
    feats = [(2.0 * g.standard_normal((T, 40))).astype(np.float32) for T in FRAMES]
    other = [(2.0 * g.standard_normal((T, 40))).astype(np.float32) for T in FRAMES]
    wavs = [synthetic_wav(n, fs, seed=n) for n, fs in WAVS]
    other_wavs = [synthetic_wav(n, fs, seed=n + 1) for n, fs in WAVS]
    paths = []
    for i, (w, (n, fs)) in enumerate(zip(wavs, WAVS)):
        paths.append(str(tmp / ("utt%d.wav" % i)))
        wavfile.write(paths[-1], fs, w)
    ref_post = [onnet3.forward(model, f) for f in feats]
    ref_feats = [of.feat_for_nnet(w.astype(np.float32), deps.lda.numpy(), samp_freq=float(fs)) for w, (n, fs) in zip(wavs, WAVS)]
    ref_wav_post = [onnet3.forward(model, f) for f in ref_feats]
    return dict(tmp=tmp, nnet_path=nnet_path, model=model, model_log=model_log, deps=deps, feats=feats, other=other, wavs=wavs,
                other_wavs=other_wavs, paths=paths, ref_post=ref_post, ref_feats=ref_feats, ref_wav_post=ref_wav_post)


def _wave_data(wavs, scale=None):
    from common import feat
    out = []
    for i, (w, (n, fs)) in enumerate(zip(wavs, WAVS)):
        x = w.astype(np.float32)
        if scale and i in scale:
            x = x * scale[i]
        out.append(feat.read_wav_kaldi_internal(x, fs))
    return out


def _mfcc_opts():
    from common import feat
    opts = feat.MfccOptions()
    opts.use_energy = False
    opts.frame_opts.allow_downsample = True
    opts.frame_opts.snip_edges = False
    return opts


def test_batch_matches_the_oracles(world):
    """Test 1: every utterance of the batch against oracle.nnet3 / oracle.feat, with the single-utterance tests' bounds."""
    import ppg
    model, deps = world["model"], world["deps"]
    out = ppg.compute_full_ppg_batch(model, [torch.from_numpy(f).cuda() for f in world["feats"]])
    assert len(out) == 4
    for T, got, ref in zip(FRAMES, out, world["ref_post"]):
        got = got.cpu().numpy()
        assert got.shape == (T, 5816)
        print("T=%d: posterior max err %.2e, row-sum err %.1e" % (T, np.abs(got - ref).max(), np.abs(got.sum(1) - 1).max()))
        assert np.abs(got - ref).max() <= 2e-6
        assert np.abs(got.sum(1) - 1.0).max() <= 1e-4
        assert np.array_equal(got.argmax(1), ref.argmax(1))
    # second batch: B = 1, T = 37, log-softmax output
    f37 = world["feats"][2]
    (logp,) = ppg.compute_full_ppg_batch(world["model_log"], [f37])
    ref = onnet3.forward(world["model_log"], f37)
    logp = logp.cpu().numpy()
    print("T=37 log-softmax: log-posterior max err %.2e, posterior max err %.2e" % (np.abs(logp - ref).max(), np.abs(np.exp(logp) - np.exp(ref)).max()))
    assert logp.shape == (37, 5816) and np.abs(logp - ref).max() <= 2e-4 and np.abs(np.exp(logp) - np.exp(ref)).max() <= 2e-6
    assert np.abs(np.exp(logp).sum(1) - 1.0).max() <= 1e-4
    # wav -> features -> full PPG, and the monophone mass
    wd = _wave_data(world["wavs"])
    fe = ppg.compute_feat_for_nnet_batch(wd, deps.lda)
    full = ppg.compute_ppg_batch(wd, deps, is_full_ppg=True)
    mono = ppg.compute_ppg_batch(wd, deps, is_full_ppg=False)
    for T, f, rf, p, rp, m in zip(FRAMES, fe, world["ref_feats"], full, world["ref_wav_post"], mono):
        f, p = f.cpu().numpy(), p.cpu().numpy()
        assert f.shape == (T, 40) and p.shape == (T, 5816) and tuple(m.shape) == (T, 40) and m.is_cuda
        print("T=%d wav: nnet-input max err %.2e, full PPG max err %.2e, monophone mass err %.1e" % (
            T, np.abs(f - rf).max(), np.abs(p - rp).max(), abs(float(m.sum()) - T)))
        assert np.abs(f - rf).max() <= 1e-4                                               # test_gpu_feat.py
        assert np.abs(p - rp).max() <= 5e-5 and np.abs(p.sum(1) - 1).max() <= 1e-4        # test_gpu_tdnn.py
        assert abs(float(m.sum()) - T) <= 1e-2


def test_utterances_do_not_see_their_neighbours(world):
    """Test 2: the batch again with utterances 0 and 3 replaced (utterance 3 scaled by 1e4); same lengths, so same column
    space and launch shapes.  Utterances 1 and 2 must come out with the same bits at every stage."""
    import ppg
    from common import feat
    deps, model = world["deps"], world["model"]
    a = _wave_data(world["wavs"])
    mixed = [world["other_wavs"][0], world["wavs"][1], world["wavs"][2], world["other_wavs"][3]]
    b = _wave_data(mixed, scale={3: 1e4})
    ma, fa = feat.compute_mfcc_feats_batch(a, _mfcc_opts())
    mb, fb = feat.compute_mfcc_feats_batch(b, _mfcc_opts())
    assert fa == fb == list(FRAMES)
    sa, sb = (feat.cmn_splice_transform_batch(m, fa, 3, 3, None) for m in (ma, mb))
    la, lb = (ppg.compute_feat_for_nnet_batch(w, deps.lda) for w in (a, b))
    pa, pb = (ppg.compute_ppg_batch(w, deps) for w in (a, b))
    qa, qb = (ppg.compute_ppg_batch(w, deps, is_full_ppg=False) for w in (a, b))
    lo, hi = FRAMES[0], FRAMES[0] + FRAMES[1] + FRAMES[2]
    assert torch.equal(ma[lo:hi], mb[lo:hi]) and not torch.equal(ma[hi:], mb[hi:]) and not torch.equal(ma[:lo], mb[:lo])
    assert torch.equal(sa[lo:hi], sb[lo:hi]) and not torch.equal(sa[hi:], sb[hi:])
    for k in (1, 2):
        assert torch.equal(la[k], lb[k]) and torch.equal(pa[k], pb[k]) and torch.equal(qa[k], qb[k]), k
    assert not torch.equal(pa[3], pb[3])          # (utterance 0 has one frame: minus its own mean it is zero whatever the wav)
    # the acoustic model alone, with feature values 1e4 times larger next door
    fa_ = [torch.from_numpy(f).cuda() for f in world["feats"]]
    fb_ = [torch.from_numpy(world["other"][0]).cuda(), fa_[1], fa_[2], torch.from_numpy(world["other"][3] * 1e4).cuda()]
    xa, xb = ppg.compute_full_ppg_batch(model, fa_), ppg.compute_full_ppg_batch(model, fb_)
    ya, yb = (ppg.compute_full_ppg_batch(model, f, deps.monophone_trans) for f in (fa_, fb_))
    for k in (1, 2):
        assert torch.equal(xa[k], xb[k]) and torch.equal(ya[k], yb[k]), k
    assert not torch.equal(xa[3], xb[3]) and all(bool(torch.isfinite(x).all()) for x in xb)


def test_batch_against_the_single_utterance_calls(world, monkeypatch):
    """Test 3 (see the module docstring for where bits are promised and where a bound is)."""
    import ppg
    from common import feat
    deps, model = world["deps"], world["model"]
    wd = _wave_data(world["wavs"])
    mf, frames = feat.compute_mfcc_feats_batch(wd, _mfcc_opts())
    fe = ppg.compute_feat_for_nnet_batch(wd, deps.lda)
    at = 0
    for w, T, f in zip(wd, frames, fe):
        assert torch.equal(mf[at:at + T], feat.compute_mfcc_feats(w, _mfcc_opts()))
        assert torch.equal(f, ppg.compute_feat_for_nnet_internal(w, deps.lda))
        at += T
    opts = _mfcc_opts()
    opts.use_energy = True
    me, _ = feat.compute_mfcc_feats_batch(wd, opts)
    assert torch.equal(me[1 + 5:1 + 5 + 37], feat.compute_mfcc_feats(wd[2], opts))
    feats = [torch.from_numpy(f).cuda() for f in world["feats"]]
    monkeypatch.delenv("FACPPG_GEMM_SHAPE", raising=False)
    single = [ppg.compute_full_ppg(model, f) for f in feats]
    monkeypatch.setenv("FACPPG_GEMM_SHAPE", "legacy")
    legacy = [ppg.compute_full_ppg(model, f) for f in feats]
    monkeypatch.delenv("FACPPG_GEMM_SHAPE")
    measured = max(float((a - b).abs().max()) for a, b in zip(single, legacy))
    # B = 1: same kernel, same sums per column -> renorm and softmax see equal inputs and give equal bits
    (one,) = ppg.compute_full_ppg_batch(model, [feats[2]])
    assert torch.equal(one, single[2])
    (one_log,) = ppg.compute_full_ppg_batch(world["model_log"], [feats[2]])
    assert torch.equal(one_log, ppg.compute_full_ppg(world["model_log"], feats[2]))
    # B = 4 (252 columns) and (150, 150) (328 columns: the 64-column kernel)
    g = np.random.Generator(np.random.PCG64(22))
    second = torch.from_numpy((2.0 * g.standard_normal((150, 40))).astype(np.float32)).cuda()
    four = ppg.compute_full_ppg_batch(model, feats)
    two = ppg.compute_full_ppg_batch(model, [feats[3], second])
    dev4 = max(float((a - b).abs().max()) for a, b in zip(four, single))
    dev2 = max(float((two[0] - single[3]).abs().max()), float((two[1] - ppg.compute_full_ppg(model, second)).abs().max()))
    print("legacy vs default (single utterance): %.3e; batch of 4 vs single: %.3e; batch (150, 150) vs single: %.3e" % (measured, dev4, dev2))
    for dev in (dev4, dev2):
        assert dev <= 2.0 * measured and dev <= 2e-6


def test_fused_monophone_output(world):
    """Test 4: the fused softmax + reduction against reduce_ppg_dim(softmax output): 1e-6 absolute per entry (sums of at
    most 5816 non-negative terms that total at most 1), rows sum to 1 within 1e-4."""
    import ppg
    model, red = world["model"], world["deps"].monophone_trans
    g = np.random.Generator(np.random.PCG64(23))
    sets = {"(1, 5, 37, 150)": [torch.from_numpy(f).cuda() for f in world["feats"]],
            "(37,)": [torch.from_numpy(world["feats"][2]).cuda()],
            "(150, 16, 17)": [torch.from_numpy((2.0 * g.standard_normal((T, 40))).astype(np.float32)).cuda() for T in (150, 16, 17)]}
    for name, feats in sets.items():
        full = ppg.compute_full_ppg_batch(model, feats)
        mono = ppg.compute_full_ppg_batch(model, feats, red)
        for f, m in zip(full, mono):
            want = ppg.reduce_ppg_dim(f, red)
            assert tuple(m.shape) == (f.shape[0], 40)
            err, row = float((m - want).abs().max()), float((m.sum(1) - 1).abs().max())
            print("frames %s, T=%d: fused vs reduce_ppg_dim %.2e, row-sum err %.1e" % (name, f.shape[0], err, row))
            assert err <= 1e-6 and row <= 1e-4
    with pytest.raises(Exception, match="softmax"):
        ppg.compute_full_ppg_batch(world["model_log"], sets["(37,)"], red)


def _loader_hparams(**kw):
    from common.hparams import create_hparams_stage
    kw.setdefault("is_full_ppg", False)
    kw.setdefault("load_feats_from_disk", False)
    return create_hparams_stage(n_symbols=40, **kw)


@pytest.fixture(scope="module")
def corpus(world):
    """Four short 16 kHz wavs (25, 37, 50 and 31 frames) and their list file."""
    tmp = world["tmp"]
    paths = []
    for i, n in enumerate((4000, 5920, 8000, 4960)):
        paths.append(str(tmp / ("train%d.wav" % i)))
        wavfile.write(paths[-1], 16000, synthetic_wav(n, 16000, seed=40 + i))
    (tmp / "train.txt").write_text("\n".join(paths) + "\n")
    return paths, str(tmp / "train.txt")


def test_ppg_mel_loader_end_to_end(world, corpus, monkeypatch):
    """Test 5."""
    import random

    import ppg
    from common import data_utils, feat, layers
    from script.train_ppg2mel import finetune, load_model
    from facppg import synth
    deps = world["deps"]
    paths, listing = corpus
    cache = str(world["tmp"] / "feats.pkl")
    hp = _loader_hparams(is_cache_feats=True, feats_cache_path=cache)
    loader = data_utils.PPGMelLoader(listing, hp, ppg_deps=deps, batch_utterances=3)         # chunks of 3 + 1
    order = list(paths)
    random.seed(hp.seed)
    random.shuffle(order)
    assert loader.data_utterance_paths == order and len(loader) == 4
    stft = layers.TacotronSTFT(hp.filter_length, hp.hop_length, hp.win_length, hp.n_acoustic_feat_dims, hp.sampling_rate, hp.mel_fmin,
                               hp.mel_fmax)
    for i, path in enumerate(order):
        x, y = loader[i]
        fs, wav = wavfile.read(path)
        mono = ppg.reduce_ppg_dim(data_utils.get_ppg(path, deps), deps.monophone_trans).cpu()
        mel = stft.mel_spectrogram(torch.from_numpy(wav.astype(np.float32) / hp.max_wav_value)[None].cuda())[0].t().cpu()
        assert x.dtype == torch.float32 and tuple(x.shape) == tuple(mono.shape) == ((len(wav) + 80) // 160, 40)
        assert tuple(y.shape) == (len(wav) // hp.hop_length + 1, hp.n_acoustic_feat_dims)     # N // hop + 1 frames, exactly
        e_p, e_m = float((x - mono).abs().max()), float((y - mel).abs().max())
        print("%s: PPG vs get_ppg + reduce %.2e, mel vs mel_spectrogram alone %.2e" % (os.path.basename(path), e_p, e_m))
        assert e_p <= 2e-6 and e_m <= 2e-6
    full = data_utils.PPGMelLoader(listing, _loader_hparams(is_full_ppg=True, ppg_subsampling_factor=2), ppg_deps=deps)
    for i, path in enumerate(order):
        whole = data_utils.get_ppg(path, deps)
        x, _ = full[i]
        assert tuple(x.shape) == ((whole.shape[0] + 1) // 2, 5816) and float((x - torch.from_numpy(whole[0::2])).abs().max()) <= 2e-6
    # cache round trip: no model, no dependencies
    back = data_utils.PPGMelLoader(listing, _loader_hparams(load_feats_from_disk=True, feats_cache_path=cache), ppg_deps=None)
    assert len(back) == 4
    for i in range(4):
        assert torch.equal(back[i][0], loader[i][0]) and torch.equal(back[i][1], loader[i][1])
    # two finetune() steps from the loader
    hp.batch_size = 2
    model = load_model(hp)
    model.load_state_dict(synth.tacotron_state_dict(hp))
    res = finetune(model.eval(), hp, loader, data_utils.ppg_acoustics_collate, 2, step_seeds=lambda s: 100 + s, log=None)
    assert len(res["losses"]) == 2 and all(np.isfinite(v) for v in res["losses"] + res["grad_norms"])


def test_synthesize_corpus_from_wavs(world, corpus, monkeypatch):
    """Test 6: --wav_list at world size 1 against a --ppg_list run over the PPGs get_ppg_batch returns, same seeds."""
    from common import data_utils
    from common.hparams import create_hparams_stage
    from facppg import synth
    from script import synthesize_corpus
    from waveglow.glow import WaveGlow
    from test_gpu_e2e import weightnorm_state_dict
    monkeypatch.setenv("FACPPG_DECODER_MODE", "coop")
    monkeypatch.setenv("FACPPG_DECODER_COOP_U", "150")
    monkeypatch.setenv("FACPPG_BILSTM_MODE", "single")
    tmp = world["tmp"]
    paths, listing = corpus
    cfg = dict(synth.WAVEGLOW_CONFIG)
    wg = WaveGlow(**cfg)
    wg.load_state_dict(weightnorm_state_dict(synth.waveglow_state_dict(cfg)), strict=True)
    torch.save({"model": wg, "iteration": 0, "optimizer": None, "learning_rate": 1e-4}, tmp / "waveglow.pt")
    hp = create_hparams_stage(n_symbols=40, is_full_ppg=False)
    torch.save({"state_dict": synth.tacotron_state_dict(hp, gate_bias=-10.0), "iteration": 0}, tmp / "tacotron.pt")
    common = ["--ppg2mel_model", str(tmp / "tacotron.pt"), "--waveglow_model", str(tmp / "waveglow.pt"), "--seed", "31",
              "--limit_steps_to_input", "--hparams", "n_symbols=40,is_full_ppg=False", "--batch_size", "3"]
    written = synthesize_corpus.main(common + ["--wav_list", listing, "--output_dir", str(tmp / "from_wav"), "--nnet_path", world["nnet_path"],
                                               "--feats_dir", KF])
    assert written == ["train%d.wav" % i for i in range(4)]
    ppg_paths = []
    for p, a in zip(paths, data_utils.get_ppg_batch(paths, world["deps"], is_full_ppg=False)):
        ppg_paths.append(os.path.join(str(tmp), os.path.basename(p)[:-4] + ".npy"))
        np.save(ppg_paths[-1], a)
    (tmp / "ppgs.txt").write_text("\n".join(ppg_paths) + "\n")
    synthesize_corpus.main(common + ["--ppg_list", str(tmp / "ppgs.txt"), "--output_dir", str(tmp / "from_ppg")])
    for i, p in enumerate(paths):
        n = wavfile.read(p)[1].shape[0]
        sr, a = wavfile.read(tmp / "from_wav" / ("train%d.wav" % i))
        assert sr == 16000 and a.shape == (((n + 80) // 160) * 160,) and np.isfinite(a).all()   # Tout_i = Tin_i frames, hop 160
        assert np.array_equal(a, wavfile.read(tmp / "from_ppg" / ("train%d.wav" % i))[1]), i
