"""script.synthesize_corpus --wav_list with and without --device_ppgs: wall clock of main(), wav list to wav files, world size 1.

32 synthetic 16 kHz wavs of 1-4 s (tools/time_wav2wav.py's signal and length law), batches of 8, the synthetic acoustic model of
tools/time_wav2wav.py (TDNN hidden 512, 5816 senones), the small synthetic checkpoints of tests/test_gpu_wav2wav.py (monophone,
n_symbols = 40) and their senone counterpart, one Synthesizer per pair.  The two commands alternate in one process, four runs
each, the first of each a warm-up.  Prints one JSON line; a file name as the first argument gets it too.

  python tools/time_corpus_wav2wav.py [OUT.json]
"""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fac-via-ppg_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
from scipy.io import wavfile

import ppg  # noqa: F401
from common import nnet3
from common.hparams import create_hparams_stage
from facppg import synth
from facppg.pipeline import Synthesizer
from script import synthesize_corpus
from waveglow.glow import WaveGlow
from test_gpu_e2e import weightnorm_state_dict

sys.path.insert(0, os.path.join(ROOT, "tools"))
from time_wav2wav import synthetic_wav

N_UTT, BATCH = 32, 8
tmp = tempfile.mkdtemp()
kf = os.path.join(ROOT, "tests", "golden", "kaldi_feats")
net = nnet3.synthetic_tdnn(input_dim=40, hidden=512, output_dim=5816, norm="renorm", seed=3, lda=False)
nnet3.write_nnet3(os.path.join(tmp, "final.raw"), net)
g = np.random.Generator(np.random.PCG64(7))
frames = (100 + g.integers(0, 301, size=N_UTT)).tolist()
paths = []
for i, n in enumerate(frames):
    paths.append(os.path.join(tmp, "utt%02d.wav" % i))
    wavfile.write(paths[-1], 16000, synthetic_wav(np, 160 * n, 900 + i))
listing = os.path.join(tmp, "wavs.txt")
open(listing, "w").write("\n".join(paths) + "\n")
cfg = dict(synth.WAVEGLOW_CONFIG)
wg = WaveGlow(**cfg)
wg.load_state_dict(weightnorm_state_dict(synth.waveglow_state_dict(cfg)), strict=True)
torch.save({"model": wg, "iteration": 0, "optimizer": None, "learning_rate": 1e-4}, os.path.join(tmp, "wg.pt"))
res = {}
for tag, hp_text, hp in (("monophone", "n_symbols=40,is_full_ppg=False", create_hparams_stage(n_symbols=40, is_full_ppg=False, max_decoder_steps=400)),
                         ("senone", "n_symbols=5816,is_full_ppg=True", create_hparams_stage(n_symbols=5816, is_full_ppg=True, max_decoder_steps=400))):
    tp = os.path.join(tmp, "taco_%s.pt" % tag)
    torch.save({"state_dict": synth.tacotron_state_dict(hp, gate_bias=-10.0), "iteration": 0}, tp)
    s = Synthesizer(tp, os.path.join(tmp, "wg.pt"), hparams=hp)
    common = ["--ppg2mel_model", tp, "--waveglow_model", os.path.join(tmp, "wg.pt"), "--seed", "31", "--limit_steps_to_input", "--hparams", hp_text,
              "--batch_size", str(BATCH), "--wav_list", listing, "--nnet_path", os.path.join(tmp, "final.raw"), "--feats_dir", kf]
    times = {"host": [], "device": []}
    for rep in range(4):          # (the first of each is the warm-up)
        for kind, extra in (("host", []), ("device", ["--device_ppgs"])):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            names = synthesize_corpus.main(common + ["--output_dir", os.path.join(tmp, "out_%s_%s" % (tag, kind))] + extra, synthesizer=s)
            torch.cuda.synchronize()
            assert len(names) == N_UTT
            if rep:
                times[kind].append(round((time.perf_counter() - t0) * 1e3, 1))
    same = all(np.array_equal(wavfile.read(os.path.join(tmp, "out_%s_host" % tag, n))[1], wavfile.read(os.path.join(tmp, "out_%s_device" % tag, n))[1])
               for n in names)
    res[tag] = dict(times, files_equal=same)
    print(tag, res[tag], flush=True)
line = json.dumps({"workload": "script.synthesize_corpus --wav_list, %d wavs of 1-4 s (%d frames), batch size %d, world size 1, TDNN hidden 512, 5816 senones, "
                               "hop 160, --limit_steps_to_input; wall clock of main() in ms, wav list to wav files, the two alternating in one process after one "
                               "warm-up run each" % (N_UTT, sum(frames), BATCH),
                   "gpu": torch.cuda.get_device_name(0), "host": "--wav_list", "device": "--wav_list --device_ppgs", "results": res})
print(line)
if len(sys.argv) > 1:
    open(sys.argv[1], "a").write(line + "\n")
