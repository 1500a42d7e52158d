"""Phase-level cycle profile of the cooperative decoder (FACPPG_DECODER_PROF=1).
Worker phases of the split decoder since round 20: every gather phase but "gather CTX" begins with the worker's pause between
publishing and polling (0.85 us by default; printed as "pause+gather ..."), and with the one-barrier stages "att LSTM" and
"dec LSTM + gather DH" contain the barrier in front of the unit's pointwise part.  Compare against earlier rounds' files
(r05, r06) with FACPPG_DECODER_STEP=legacy, which has neither.  The main workgroup's "query weights requested" varies by
about 0.5 us between builds and runs of the same code."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fac-via-ppg_amd")]
os.environ["FACPPG_DECODER_PROF"] = "1"
import torch
from common.hparams import create_hparams_stage
from facppg import synth, pipeline
from script.train_ppg2mel import load_model
Tin = 200
hp = create_hparams_stage(max_decoder_steps=Tin)
m = load_model(hp); m.load_state_dict(synth.tacotron_state_dict(hp)); m.eval()
x, _ = pipeline.pad_ppgs([synth.synthetic_ppg(Tin)])
x = x.cuda()
for i in range(3):
    torch.cuda.synchronize(); t = time.perf_counter(); m.inference(x, seed=1); torch.cuda.synchronize()
    print("inference %.2f ms" % ((time.perf_counter() - t) * 1e3))
