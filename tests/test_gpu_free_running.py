"""GPU: script.train_ppg2mel.validate_free_running, finetune(free_running=True) and the script.validate_ppg2mel command line.

A synthetic model (create_hparams_stage(n_symbols=40, max_decoder_steps=48), synth.tacotron_state_dict) and five utterances built
like forced_helpers.forced_utterances, Tin 12 to 40, in batches of 2 -- so the last batch is a batch of one.
validate_free_running must equal, bit for bit, a loop written out here that makes the same inference calls with the same
utterance_seeds and step_limits and then calls mel_dtw and attention_path; what those two compute is held to the float64
references in test_gpu_mel_dtw.py."""
import math
import pickle
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TIN = (12, 40, 25, 33, 18)
TOUT = (20, 44, 31, 38, 27)
MAX_STEPS = 48


def _hparams(**kw):
    from common.hparams import create_hparams_stage
    return create_hparams_stage(n_symbols=40, max_decoder_steps=MAX_STEPS, **kw)


def _utterances():
    """(PPG [L_in, 40], acoustic [L_out, 80]) pairs as a data set yields them, NOT sorted by length."""
    from facppg import synth
    return [(torch.from_numpy(synth.synthetic_ppg(li, 40, seed=s, alpha=0.1)).float(), synth.synthetic_mel(1, lo, seed=100 + s)[0].t().contiguous())
            for s, (li, lo) in enumerate(zip(TIN, TOUT))]


def _model(hp, gate_bias=-10.0):
    from facppg import synth
    from script.train_ppg2mel import load_model
    m = load_model(hp)
    m.load_state_dict(synth.tacotron_state_dict(hp, seed=16807, gate_bias=gate_bias))
    return m.eval()


def _by_hand(model, items, batch_size, seed, step_factor):
    """The loop validate_free_running is defined by -> rows of (frames, limit, mel_dtw's dict row, attention_path's dict row)."""
    from facppg import score
    rows = []
    with torch.no_grad():
        for at in range(0, len(items), batch_size):
            part = items[at:at + batch_size]
            tin, ttgt = [int(p.shape[0]) for p, _ in part], [int(m.shape[0]) for _, m in part]
            x, y = torch.zeros(len(part), 40, max(tin)), torch.zeros(len(part), 80, max(ttgt))
            for b, (p, m) in enumerate(part):
                x[b, :, :tin[b]] = p.t()
                y[b, :, :ttgt[b]] = m.t()
            limits = [MAX_STEPS if step_factor is None else min(MAX_STEPS, int(math.ceil(step_factor * t))) for t in ttgt]
            out = model.inference(x.cuda(), lengths=tin, utterance_seeds=[seed + at + b for b in range(len(part))], step_limits=limits)
            frames = [int(v) for v in out.out_lengths]
            dtw = score.mel_dtw(out[1], frames, y.cuda(), ttgt, n_cep=13, band=0)
            path = score.attention_path(out[3], frames, tin)
            for b in range(len(part)):
                rows.append((frames[b], limits[b], {k: v[b] for k, v in dtw.items()}, {k: v[b] for k, v in path.items()}))
    return rows


def _same(result, rows):
    from script.train_ppg2mel import FREE_RUNNING_FIELDS
    assert all(len(result[name]) == len(rows) for name in FREE_RUNNING_FIELDS)
    for k, (frames, limit, dtw, path) in enumerate(rows):
        assert int(result["frames"][k]) == frames and int(result["target_frames"][k]) == TOUT[k], k
        assert bool(result["stopped"][k]) == (frames < limit), (k, frames, limit)
        for name in ("mcd", "stretch"):
            assert result[name][k].tobytes() == dtw[name].tobytes(), (k, name, result[name][k], dtw[name])
        for name in FREE_RUNNING_FIELDS[5:]:
            assert result[name][k].tobytes() == path[name].tobytes(), (k, name, result[name][k], path[name])
    assert result["mean_mcd"] == float(result["mcd"].mean()) and result["stopped_share"] == float(result["stopped"].mean())
    assert result["mean_coverage"] == float(result["coverage"].mean())


def test_equals_the_loop_written_out(capsys):
    from script.train_ppg2mel import validate_free_running
    items = _utterances()
    model = _model(_hparams())                        # the gate stays shut: every utterance runs into its limit
    res = validate_free_running(model, items, 2, seed=7, iteration=3)
    assert "Free-running 3: MCD %.4f dB, stopped 0.000, coverage %.3f" % (res["mean_mcd"], res["mean_coverage"]) in capsys.readouterr().out
    _same(res, _by_hand(model, items, 2, 7, None))
    assert res["frames"].tolist() == [MAX_STEPS] * 5 and not res["stopped"].any()
    assert np.isfinite(res["mcd"]).all() and (res["mcd"] > 0).all() and (res["visited"] >= 1).all()
    assert not model.training
    # the rows are the utterances' own, in valset order: each one alone (batch size 1) gives the same row, and another seed another one
    alone = validate_free_running(model, items, 1, seed=7, rank=1)
    assert capsys.readouterr().out.count("Free-running") == 0
    assert all(alone[k].tobytes() == res[k].tobytes() for k in ("frames", "mcd", "stretch", "visited", "focus", "last"))
    assert validate_free_running(model, items, 2, seed=8, rank=1)["mcd"].tobytes() != res["mcd"].tobytes()
    # step_factor = 0.5 caps every utterance at ceil(0.5 * target) frames; the mode the model was found in comes back
    model.train()
    half = validate_free_running(model, items, 2, seed=7, step_factor=0.5, rank=1)
    assert model.training
    model.eval()
    assert half["frames"].tolist() == [int(math.ceil(0.5 * t)) for t in TOUT] and not half["stopped"].any()
    _same(half, _by_hand(model, items, 2, 7, 0.5))


def test_stopped_follows_the_gate():
    """An open gate (bias 0): utterances stop on their own before the limit, and ``stopped`` says which."""
    from script.train_ppg2mel import validate_free_running
    items = _utterances()
    model = _model(_hparams(), gate_bias=0.0)
    res = validate_free_running(model, items, 2, seed=1, rank=1)
    rows = _by_hand(model, items, 2, 1, None)
    _same(res, rows)
    print("open gate: frames %s, stopped %s" % (res["frames"].tolist(), res["stopped"].tolist()))
    assert res["stopped"].tolist() == [r[0] < MAX_STEPS for r in rows]


class Utterances(torch.utils.data.Dataset):
    def __init__(self, items):
        self.items = items

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def test_finetune_scores_every_checkpoint(tmp_path):
    from common.data_utils import ppg_acoustics_collate
    from script.train_ppg2mel import FREE_RUNNING_FIELDS, finetune
    items = _utterances()
    runs = {}
    for flag in (True, False):
        hp = _hparams(batch_size=2, iters_per_checkpoint=1)
        runs[flag] = finetune(_model(hp), hp, Utterances(items), ppg_acoustics_collate, 2, output_directory=str(tmp_path / ("run%d" % flag)),
                              valset=Utterances(items), step_seeds=lambda s: 100 + s, log=None, free_running=flag)
    scored = runs[True]["free_running"]
    assert [it for it, _ in scored] == [0, 1] and runs[False]["free_running"] == []
    for _, res in scored:
        assert all(len(res[name]) == 5 for name in FREE_RUNNING_FIELDS) and res["target_frames"].tolist() == list(TOUT)
        assert np.isfinite(res["mean_mcd"])
    assert scored[0][1]["mcd"].tobytes() != scored[1][1]["mcd"].tobytes()           # the second checkpoint is another model
    assert runs[True]["losses"] == runs[False]["losses"] and runs[True]["grad_norms"] == runs[False]["grad_norms"]


def test_command_line(tmp_path, capsys):
    from facppg import synth
    from script import validate_ppg2mel
    from script.train_ppg2mel import validate_free_running
    items = _utterances()
    cache, listing, ckpt, out = (str(tmp_path / n) for n in ("feats.pkl", "val.txt", "checkpoint_0", "scores.tsv"))
    with open(cache, "wb") as f:
        pickle.dump([[p.numpy() for p, _ in items], [m for _, m in items]], f)
    paths = ["utt%d.wav" % k for k in range(5)]
    open(listing, "w").write("\n".join(paths) + "\n")
    hp = _hparams()
    torch.save({"iteration": 0, "state_dict": synth.tacotron_state_dict(hp, seed=16807, gate_bias=-10.0), "optimizer": {}, "learning_rate": 1e-4}, ckpt)
    loss, res = validate_ppg2mel.main(["--ppg2mel_model", ckpt, "--wav_list", listing, "--batch_size", "2", "--seed", "7", "--step_factor", "0.75",
                                       "--out", out, "--hparams",
                                       "n_symbols=40,max_decoder_steps=%d,load_feats_from_disk=True,feats_cache_path=%s" % (MAX_STEPS, cache)])
    printed = capsys.readouterr().out
    assert "Validation loss 0:" in printed and "Free-running 0: MCD" in printed and np.isfinite(loss)
    want = validate_free_running(_model(hp), items, 2, seed=7, step_factor=0.75, rank=1)
    shuffled = list(paths)
    random.seed(hp.seed)
    random.shuffle(shuffled)                           # PPGMelLoader's order of the list; the cache holds the features in that order
    lines = open(out).read().splitlines()
    assert len(lines) == 5
    for k, line in enumerate(lines):
        cells = line.split("\t")
        assert len(cells) == 12 and cells[0] == shuffled[k]
        assert line == validate_ppg2mel.score_line(shuffled[k], want, k), (k, line)
        assert int(cells[1]) == TOUT[k] and int(cells[2]) == int(math.ceil(0.75 * TOUT[k])) and cells[3] == "0"
        assert all(np.isfinite(float(c)) for c in cells[1:])
    assert all(res[k].tobytes() == want[k].tobytes() for k in ("mcd", "frames", "focus"))
