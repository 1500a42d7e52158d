"""CPU: the per-phone report without a device -- the float64 reference of align_helpers.py against its float32 restatement over
the matrix T in (1, 2, 7, 63, 64, 65, 150, 600) x D in (3, 40), the self-consistency of the definition (x force-aligned to its own
decoded runs gives those runs back), the hand cases of the forced alignment, the TextGrid writer and the phone table, every
host-side refusal of the three entry points (nothing is launched: no device is needed) and the corpus script's flags."""
import ctypes
import os
import re

import numpy as np
import pytest

import align_helpers as ah
from conftest import ROOT
from facppg import lib as flib

EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -4
PHONES = os.path.join(ROOT, "tests", "golden", "arpa_phonemes")
NAMES = ("facppg_ppg_emissions", "facppg_ppg_decode_phones_workspace_bytes", "facppg_ppg_decode_phones", "facppg_ppg_force_align_workspace_bytes",
         "facppg_ppg_force_align")


def test_header_declares_and_library_exports_the_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "facppg.h")).read(), flags=re.S)
    L = flib.load()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(L, name) and name in flib.exported_symbols()


@pytest.mark.parametrize("D", ah.DIMS_CPU)
def test_float32_restatement_equals_the_float64_reference_and_the_definition_is_self_consistent(D):
    for T in ah.FRAMES:
        c = ah.case(T, D)
        (l64, c64, a64), (l32, c32, a32) = c[np.float64], c[np.float32]
        assert np.array_equal(l64, l32), (T, D)
        runs = ah.runs_of(l64)
        for a in (a64, a32):
            # force-aligning x to its own decoded runs reproduces the runs' boundaries: a better alignment would be a better decode
            assert a["ok"] and a["start"].tolist() == [r[1] for r in runs] and a["frames"].tolist() == [r[2] for r in runs], (T, D)
            assert (a["gop"] <= 0).all() and (a["hits"] <= a["frames"]).all()
        assert np.array_equal(a64["hits"], a32["hits"])
        gap = abs(float(c64) - (len(runs) - 1) * ah.SWITCH_COST - float(a64["cost"]))
        assert gap < 5e-13, (T, D, gap)
        assert abs(float(c32) - float(c64)) <= ah.cost_deviation_per_frame() * T
    print("D = %d: float32 restatement: worst |cost32 - cost64| / T = %.3e; -log deviation %.3e (emission tolerance %.3e)" % (
        D, ah.cost_deviation_per_frame(), ah.emission_deviation(), ah.emission_tolerance()))
    assert 0.0 < ah.emission_deviation() < 1e-6


def test_float32_and_float64_decode_the_same_labels_at_every_width_the_gpu_test_uses():
    """The GPU test holds the device's labels to both: D = 256 is not in the matrix above."""
    for D in ah.DIMS_GPU:
        for T in ah.FRAMES:
            c = ah.case(T, D)
            assert np.array_equal(c[np.float64][0], c[np.float32][0]), (T, D)


def test_hand_cases_of_the_forced_alignment():
    for name, x, seq, opt, want in ah.hand_cases():
        for dtype in (np.float64, np.float32):
            em, eb, top = ah.emissions(x, ah.FLOOR, dtype)
            got = ah.align(em, eb, top, seq, opt)
            ah.check_expected(name, got, want)
            assert got["gop"].dtype == dtype and (got["gop"] <= 0).all()
            if not want["ok"]:
                assert np.isinf(got["cost"])
    for S in (64, 65, 1024):
        x, seq, opt = ah.long_case(S)
        r64 = ah.align(*ah.emissions(x), seq, opt)
        r32 = ah.align(*ah.emissions(x, ah.FLOOR, np.float32), seq, opt)
        assert r64["ok"] and r32["ok"] and int(r64["frames"].sum()) == 1030
        assert all((r64["frames"][i] > 0) or opt[i] for i in range(S))       # only optional states are skipped


def test_decode_hand_example():
    """Three classes; the switch cost decides whether one odd frame becomes a phone of its own."""
    x = ah.peaked([0, 0, 1, 0, 0], 3, hot=0.8)         # -log 0.8 = 0.223, -log 0.1 = 2.303: the odd frame is worth 2.08 nats
    em = ah.emissions(x)[0]
    assert ah.decode(em, 2.0)[0].tolist() == [0] * 5   # two switches cost 4 > 2.08
    assert ah.decode(em, 1.0)[0].tolist() == [0, 0, 1, 0, 0]
    labels, cost = ah.decode(em, 0.0)
    assert labels.tolist() == [0, 0, 1, 0, 0] and abs(cost - 5 * -np.log(0.8)) < 1e-6
    # a floor case: posteriors of exactly 0 give -log(floor)
    z = np.zeros((3, 2), dtype=np.float32)
    e32 = ah.emissions(z, ah.FLOOR, np.float32)[0]
    assert (e32 == -np.log(np.float32(1e-10))).all() and ah.emissions(z)[2].tolist() == [0, 0]


def test_phone_table_and_textgrid(tmp_path):
    from facppg import align
    names = align.read_phone_table(PHONES)
    assert len(names) == 40 and names[0] == "aa" and names[39] == "sil" and names[28] == "s"
    T, D, shift = 150, 40, 0.01
    runs = np.asarray(ah.runs_of(ah.case(T, D)[np.float64][0]), dtype=np.int32)
    path = str(tmp_path / "utt.TextGrid")
    align.write_textgrid(path, runs, shift, names)
    text = open(path).read()
    assert text.startswith('File type = "ooTextFile"\nObject class = "TextGrid"\n')
    assert 'class = "IntervalTier"' in text and "intervals: size = %d" % len(runs) in text
    lo = [float(v) for v in re.findall(r"^ {12}xmin = (\S+)$", text, flags=re.M)]
    hi = [float(v) for v in re.findall(r"^ {12}xmax = (\S+)$", text, flags=re.M)]
    texts = re.findall(r'^ {12}text = "(.*)"$', text, flags=re.M)
    assert len(lo) == len(hi) == len(texts) == len(runs)
    assert lo[0] == 0.0 and hi[-1] == pytest.approx(T * shift) and lo[1:] == hi[:-1]          # contiguous from 0 to T * shift
    assert lo == pytest.approx([r[1] * shift for r in runs]) and texts == [names[r[0]] for r in runs]
    assert re.search(r"^xmax = (\S+)$", text, flags=re.M).group(1) == repr(round(T * shift, 9))
    # a skipped state is left out, a gap becomes an interval without text, an overlap is refused
    align.write_textgrid(path, [(39, -1, 0), (3, 0, 4), (5, 6, 2)], shift)
    text = open(path).read()
    assert re.findall(r'^ {12}text = "(.*)"$', text, flags=re.M) == ["3", "", "5"] and "intervals: size = 3" in text
    with pytest.raises(flib.FacppgError, match="starts inside"):
        align.write_textgrid(path, [(3, 0, 4), (5, 3, 2)], shift)
    bad = tmp_path / "bad_table"
    bad.write_text("aa 0\nae 2\n")
    with pytest.raises(flib.FacppgError, match="indices"):
        align.read_phone_table(str(bad))


def test_teacher_sequence_marks_and_adds_silence():
    from facppg import align
    runs = np.asarray([(39, 0, 3), (5, 3, 4), (39, 7, 2), (8, 9, 1)], dtype=np.int32)
    cls, opt, start, frames = align.teacher_sequence(runs, 39, 10)
    assert cls.tolist() == [39, 5, 39, 8, 39] and opt.tolist() == [1, 0, 1, 0, 1]
    assert start.tolist() == [0, 3, 7, 9, 10] and frames.tolist() == [3, 4, 2, 1, 0]
    cls, opt, start, frames = align.teacher_sequence(np.asarray([(5, 0, 6)], dtype=np.int32), 39, 6)
    assert cls.tolist() == [39, 5, 39] and opt.tolist() == [1, 0, 1] and frames.tolist() == [0, 6, 0] and start.tolist() == [0, 0, 6]
    cls, opt, _, _ = align.teacher_sequence(np.asarray([(39, 0, 6)], dtype=np.int32), 39, 6)
    assert cls.tolist() == [39] and opt.tolist() == [1]
    assert align.labels_to_runs([4, 4, 1, 1, 1, 4]).tolist() == [[4, 0, 2], [1, 2, 3], [4, 5, 1]]


def _fake(k, null):
    return ctypes.c_void_p(0 if null == k else 0x1000 * (k + 1))


def _emissions(L, B=2, D=40, Tmax=9, off=(0, 9, 12), floor=1e-10, null=None):
    cfg = None if null == "cfg" else flib.AlignConfig(floor, 2.0)
    rc = L.facppg_ppg_emissions(cfg, _fake(0, null), B, D, Tmax, _fake(1, null), None if null == "host" else flib.offsets_array(off), _fake(2, null),
                                _fake(3, null), _fake(4, null), None)
    return rc, L.facppg_last_error().decode()


def _decode(L, B=2, D=40, off=(0, 9, 12), switch_cost=2.0, ws_bytes=None, null=None):
    cfg = None if null == "cfg" else flib.AlignConfig(1e-10, switch_cost)
    if ws_bytes is None:
        ws_bytes = 1 << 20
    rc = L.facppg_ppg_decode_phones(cfg, _fake(0, null), _fake(1, null), None if null == "host" else flib.offsets_array(off), B, D, _fake(2, null),
                                    _fake(3, null), _fake(4, null), ws_bytes, None)
    return rc, L.facppg_last_error().decode()


def _align(L, B=2, D=40, off=(0, 9, 12), seq=(1, 39, 2, 39, 5), opt=(0, 1, 0, 1, 0), soff=(0, 3, 5), ws_bytes=None, null=None):
    seq_h, opt_h = np.asarray(seq, dtype=np.int32), np.asarray(opt, dtype=np.uint8)
    host = lambda name, arr: None if null == name else arr.ctypes.data_as(ctypes.c_void_p)    # noqa: E731
    if ws_bytes is None:
        ws_bytes = 1 << 22
    rc = L.facppg_ppg_force_align(_fake(0, null), _fake(1, null), _fake(2, null), _fake(3, null), None if null == "off_host" else flib.offsets_array(off),
                                  B, D, _fake(4, null), host("seq_host", seq_h), _fake(5, null), host("opt_host", opt_h), _fake(6, null),
                                  None if null == "soff_host" else flib.offsets_array(soff), _fake(7, null), _fake(8, null), _fake(9, null),
                                  _fake(10, null), _fake(11, null), _fake(12, null), _fake(13, null), ws_bytes, None)
    return rc, L.facppg_last_error().decode()


def test_host_side_refusals():
    """Made-up device addresses: every refusal comes before the first launch, so none is touched."""
    L = flib.load()
    for null in list(range(5)) + ["cfg", "host"]:
        rc, msg = _emissions(L, null=null)
        assert rc == EINVAL and "NULL" in msg, (null, rc, msg)
        rc, msg = _decode(L, null=null)
        assert rc == EINVAL and "NULL" in msg, (null, rc, msg)
    for null in list(range(14)) + ["off_host", "seq_host", "opt_host", "soff_host"]:
        rc, msg = _align(L, null=null)
        assert rc == EINVAL and "NULL argument" in msg, (null, rc, msg)
    for call in (_emissions, _decode, _align):
        rc, msg = call(L, D=257)
        assert rc == EUNSUPPORTED and "got 257" in msg and "monophone" in msg, (rc, msg)
        rc, msg = call(L, D=0)
        assert rc == EINVAL and "must be positive" in msg, (rc, msg)
        rc, msg = call(L, off=(0, 9, 9))
        assert rc == EINVAL and "offsets must increase" in msg, (rc, msg)
        rc, msg = call(L, off=(1, 9, 12))
        assert rc == EINVAL and "start at 0" in msg, (rc, msg)
    rc, msg = _emissions(L, Tmax=8)
    assert rc == EINVAL and "utterance 0 has 9 frames" in msg and "Tmax = 8" in msg, (rc, msg)
    for floor in (0.0, -1.0, 2.0):
        rc, msg = _emissions(L, floor=floor)
        assert rc == EINVAL and "floor" in msg, (floor, rc, msg)
    rc, msg = _decode(L, switch_cost=-0.5)
    assert rc == EINVAL and "switch_cost" in msg, (rc, msg)
    need = L.facppg_ppg_decode_phones_workspace_bytes(12, 40)
    assert need >= 12 * 40
    rc, msg = _decode(L, ws_bytes=need - 1)
    assert rc == EWORKSPACE and str(need - 1) in msg and str(need) in msg, (rc, msg)
    assert L.facppg_ppg_decode_phones_workspace_bytes(0, 40) == 0 and "got 0, 40" in L.facppg_last_error().decode()
    assert L.facppg_ppg_decode_phones_workspace_bytes(12, 257) == 0
    # the forced alignment's own
    rc, msg = _align(L, seq=(1, 39, 2, 40, 5))
    assert rc == EINVAL and "utterance 1, state 0: class 40 is outside [0, 40)" in msg, (rc, msg)
    rc, msg = _align(L, seq=(1, -1, 2, 39, 5))
    assert rc == EINVAL and "class -1" in msg, (rc, msg)
    rc, msg = _align(L, opt=(0, 1, 1, 1, 0))
    assert rc == EINVAL and "utterance 0: states 1 and 2 are both optional" in msg, (rc, msg)
    rc, msg = _align(L, opt=(0, 1, 0, 1, 1))
    assert rc == EINVAL and "utterance 1: states 0 and 1 are both optional" in msg, (rc, msg)
    rc, msg = _align(L, soff=(0, 5, 5))
    assert rc == EINVAL and "utterance 1 has 0 states" in msg, (rc, msg)
    rc, msg = _align(L, soff=(1, 3, 5))
    assert rc == EINVAL and "start at 0" in msg, (rc, msg)
    many = 1025
    rc, msg = _align(L, B=1, off=(0, 2000), seq=(1,) * many, opt=(0,) * many, soff=(0, many))
    assert rc == EUNSUPPORTED and "1025 states" in msg and "1024" in msg, (rc, msg)
    need = L.facppg_ppg_force_align_workspace_bytes(12, 3)
    assert need >= 12 * 3
    rc, msg = _align(L, ws_bytes=need - 1)
    assert rc == EWORKSPACE and str(need - 1) in msg and str(need) in msg, (rc, msg)
    assert L.facppg_ppg_force_align_workspace_bytes(12, 1025) == 0 and "got 12, 1025" in L.facppg_last_error().decode()


def test_python_refusals_need_no_device():
    import torch
    from facppg import align
    with pytest.raises(flib.FacppgError, match="must be a GPU tensor"):
        align.decode_phones(torch.zeros(1, 4, 3), [3])
    with pytest.raises(flib.FacppgError, match="must be a GPU tensor"):
        align.force_align(torch.zeros(1, 4, 3), [3], [[0]])
    with pytest.raises(flib.FacppgError, match="equal B and D"):
        align.phone_report(torch.zeros(1, 4, 3), [3], torch.zeros(2, 4, 3), [3, 3])
    with pytest.raises(flib.FacppgError, match="sil_class"):
        align.phone_report(torch.zeros(1, 4, 3), [3], torch.zeros(1, 4, 3), [3], sil_class=4)


def test_phone_file_flags_at_parse_time(capsys):
    from script import synthesize_corpus
    base = ["--ppg2mel_model", "t.pt", "--waveglow_model", "w.pt", "--output_dir", "out"]
    with pytest.raises(SystemExit) as e:
        synthesize_corpus.parse(base + ["--ppg_list", "ppgs.txt", "--phone_file", "phones.tsv"])
    assert e.value.code == 2 and "--wav_list" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        synthesize_corpus.parse(base + ["--wav_list", "wavs.txt", "--phone_table", PHONES])       # a table without a phone file
    args = synthesize_corpus.parse(base + ["--wav_list", "wavs.txt", "--phone_file", "phones.tsv", "--phone_table", PHONES])
    assert args.phone_file == "phones.tsv" and args.phone_table == PHONES and args.score_file is None
    plain = synthesize_corpus.parse(base + ["--wav_list", "wavs.txt"])
    assert plain.phone_file is None and plain.phone_table is None
    from facppg import align
    r = np.zeros(2, dtype=align.REPORT_DTYPE)
    r["phone"], r["start"], r["frames"], r["gop"], r["share"], r["kept"] = [39, 3], [-1, 0], [0, 7], [0.0, -0.25], [0.0, 1.0], [False, True]
    assert align.phone_lines("a.wav", r, align.read_phone_table(PHONES)) == ["a.wav\t0\tsil\t0\t0\t-1\t0\t0\t0\t0", "a.wav\t1\tao\t0\t0\t0\t7\t-0.25\t1\t1"]
    assert align.phone_lines("a.wav", r)[1].split("\t")[2] == "3"
