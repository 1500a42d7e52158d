"""CPU: which kernel, in what shape, the Tacotron entry points launch -- facppg_taco_launch_plan, the host-side decision of
facppg_taco_encode (its BiLSTM), facppg_taco_decode and facppg_taco_decode_forced (csrc/facppg_taco_plan.h), at the
reference's layer widths (create_hparams_stage(): P = A = D = 300, E = 600, 80 mels, attention 150 / 32 filters of 31 taps) and
the MI355X's 240 co-resident workgroups.  The expected values are worked out by hand from the launch code as it stood before
the planning header existed:
  slices   ceil(300 / U) workgroups per utterance for U = 8, 20, 40, 75, 150 -> 38, 15, 8, 4, 2; 75 split workers of 4 units
  LDS      decoder state 17848 + 3 Tin floats; the split decoder's main workgroup adds a 16384-float stash and as many
           8192-byte query-weight rows as fit under 162816 bytes (at most 24); a worker set holds 4352 floats per utterance
           (the padded layout: 32 * (44 + 44 + 36 + 12); the legacy layout has 3680) + 1024"""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from facppg import lib as flib

ENCODE, DECODE, FORCED = 0, 1, 2
EINVAL, EUNSUPPORTED = -1, -2
SWITCHES = ("FACPPG_DECODER_MODE", "FACPPG_DECODER_COOP_U", "FACPPG_DECODER_NO_SPLIT", "FACPPG_DECODER_SPLIT_MAX_NU",
            "FACPPG_DECODER_STEP", "FACPPG_DECODER_QRES", "FACPPG_DECODER_PAUSE", "FACPPG_DECODER_NO_ROWS", "FACPPG_DECODER_PROF",
            "FACPPG_BILSTM_MODE", "FACPPG_BILSTM_STEP", "FACPPG_FORCED_NO_REGW")
STATE = 17848               # floats of the decoder's LDS state at Tin = 0
MAIN = (17860 + 16384) * 4  # Tin = 3: the state rounded up to 4 floats + attn_energy_pre's stash, bytes


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def reference_config():
    from common.hparams import create_hparams_stage
    hp = create_hparams_stage()
    c = flib.TacoConfig()
    for k, _ in flib.TacoConfig._fields_:
        if k == "bn_eps":
            c.bn_eps = 1e-5
        elif k == "attention_window_size":
            c.attention_window_size = -1 if hp.attention_window_size is None else int(hp.attention_window_size)
        else:
            setattr(c, k, getattr(hp, k))
    assert (c.prenet_dim, c.attention_rnn_dim, c.decoder_rnn_dim, c.encoder_embedding_dim) == (300, 300, 300, 600)
    assert (c.n_acoustic_feat_dims, c.attention_dim, c.attention_location_n_filters, c.attention_location_kernel_size) == (80, 150, 32, 31)
    return c


def plan(what, B, Tin=3, steps=4, wgs=0, limit=240, rc=0):
    r = flib.TacoLaunchReport()
    got = flib.load().facppg_taco_launch_plan(reference_config(), limit, what, B, Tin, steps, wgs, r)
    assert got == rc, (got, flib.load().facppg_last_error())
    return r


def shape(r):
    return (r.mode, r.nu, r.workgroups, r.launches, list(r.first_u), list(r.last_u))


def test_decode_follows_the_batch():
    r = plan(DECODE, 1)
    assert shape(r) == (2, 1, 76, 1, [4, 4], [4, 4]) and r.step == 1 and r.streamed_possible == 1
    # three query-weight rows fit next to the main workgroup's state: (162816 - 136976) // 8192
    assert (r.q_res, r.pause, r.dbg_flags, r.prof, r.lds_bytes) == (3, 16, 0, 0, MAIN + 3 * 8192)
    assert (r.first_utts, r.last_utts) == (1, 1)
    assert shape(plan(DECODE, 3)) == (2, 1, 228, 1, [4, 4], [4, 4])
    assert shape(plan(DECODE, 4)) == (2, 2, 154, 1, [4, 4], [4, 4])
    assert shape(plan(DECODE, 6)) == (2, 2, 231, 1, [4, 4], [4, 4])
    assert shape(plan(DECODE, 7)) == (2, 3, 234, 1, [4, 4], [4, 4])
    r = plan(DECODE, 9)
    assert shape(r) == (2, 3, 234, 1, [4, 4], [4, 4]) and r.streamed_possible == 0
    r = plan(DECODE, 10)
    assert shape(r) == (1, 0, 150, 1, [20, 20], [20, 20]) and r.step == 0 and r.lds_bytes == (STATE + 9) * 4
    assert (r.q_res, r.pause, r.streamed_possible) == (0, 0, 0)
    assert shape(plan(DECODE, 6, wgs=228)) == (2, 3, 156, 1, [4, 4], [4, 4])       # 3 * 77 > 228: two sets of three
    assert shape(plan(DECODE, 16)) == (1, 0, 240, 1, [20, 20], [20, 20])
    assert shape(plan(DECODE, 17)) == (1, 0, 136, 1, [40, 40], [40, 40])
    assert shape(plan(DECODE, 30)) == (1, 0, 240, 1, [40, 40], [40, 40])
    assert shape(plan(DECODE, 60)) == (1, 0, 240, 1, [75, 75], [75, 75])
    assert shape(plan(DECODE, 120)) == (1, 0, 240, 1, [150, 150], [150, 150])
    r = plan(DECODE, 121)
    assert shape(r) == (1, 0, 38, 2, [150, 150], [8, 8]) and (r.first_utts, r.last_utts) == (120, 1)
    r = plan(DECODE, 250)
    assert shape(r) == (1, 0, 150, 3, [150, 150], [20, 20]) and (r.first_utts, r.last_utts) == (120, 10)


def test_decode_follows_the_workgroup_bound():
    assert shape(plan(DECODE, 2, wgs=80)) == (2, 2, 77, 1, [4, 4], [4, 4])
    assert shape(plan(DECODE, 3, wgs=80)) == (2, 3, 78, 1, [4, 4], [4, 4])
    assert shape(plan(DECODE, 3, wgs=1000)) == (2, 1, 228, 1, [4, 4], [4, 4])      # a bound beyond the device's is none
    assert shape(plan(DECODE, 4, wgs=80)) == (1, 0, 60, 1, [20, 20], [20, 20])
    assert shape(plan(DECODE, 3, wgs=2)) == (1, 0, 2, 3, [150, 150], [150, 150])
    r = plan(DECODE, 5, limit=0)
    assert shape(r) == (0, 0, 5, 1, [0, 0], [0, 0]) and r.step == 0 and r.lds_bytes == (STATE + 9) * 4
    assert shape(plan(DECODE, 5, wgs=1)) == (0, 0, 5, 1, [0, 0], [0, 0])             # not even the widest slices (2 workgroups)


def test_decode_lds_bounds_tin():
    assert plan(DECODE, 1, Tin=200).q_res == 2             # (162816 - (18448 + 16384) * 4) // 8192
    assert plan(DECODE, 1, Tin=2157).q_res == 0            # the stash still fits, no row does
    r = plan(DECODE, 1, Tin=2158)                          # the main workgroup no longer fits: the launch asks for what it needs
    assert r.mode == 2 and r.q_res == 0 and r.lds_bytes == (24324 + 16384) * 4
    assert plan(DECODE, 1, Tin=7618).lds_bytes > 0
    plan(DECODE, 1, Tin=7619, rc=EUNSUPPORTED)
    assert b"exceeds LDS" in flib.load().facppg_last_error()
    plan(FORCED, 1, Tin=2157)
    plan(FORCED, 1, Tin=2158, rc=EUNSUPPORTED)
    plan(DECODE, 1, Tin=8193, rc=EUNSUPPORTED)


def test_decoder_mode_and_slice_width_switches(monkeypatch):
    monkeypatch.setenv("FACPPG_DECODER_MODE", "split")
    assert plan(DECODE, 9).mode == 2
    plan(DECODE, 10, rc=EUNSUPPORTED)
    assert b"split decoder needs a small batch" in flib.load().facppg_last_error()
    monkeypatch.setenv("FACPPG_DECODER_MODE", "coop")
    assert shape(plan(DECODE, 1)) == (1, 0, 38, 1, [8, 8], [8, 8])
    plan(DECODE, 1, limit=0, rc=EUNSUPPORTED)
    assert b"coop decoder needs B <= 120" in flib.load().facppg_last_error()
    monkeypatch.setenv("FACPPG_DECODER_COOP_U", "75")
    assert shape(plan(DECODE, 2)) == (1, 0, 8, 1, [75, 75], [75, 75])
    plan(DECODE, 61, rc=EUNSUPPORTED)                        # a forced width is not chunked
    monkeypatch.setenv("FACPPG_DECODER_MODE", "single")
    assert shape(plan(DECODE, 2)) == (0, 0, 2, 1, [0, 0], [0, 0])
    monkeypatch.delenv("FACPPG_DECODER_MODE")
    monkeypatch.setenv("FACPPG_DECODER_COOP_U", "150")
    assert shape(plan(DECODE, 16, wgs=32)) == (1, 0, 32, 1, [150, 150], [150, 150])
    assert plan(DECODE, 1).mode == 2                         # the width alone does not take the split shape away
    monkeypatch.setenv("FACPPG_DECODER_COOP_U", "9")         # no such width
    assert plan(DECODE, 1).mode == 0


def test_split_switches(monkeypatch):
    monkeypatch.setenv("FACPPG_DECODER_NO_SPLIT", "0")       # presence counts, not the value
    assert shape(plan(DECODE, 1)) == (1, 0, 38, 1, [8, 8], [8, 8])
    monkeypatch.delenv("FACPPG_DECODER_NO_SPLIT")
    monkeypatch.setenv("FACPPG_DECODER_SPLIT_MAX_NU", "1")
    assert shape(plan(DECODE, 4)) == (1, 0, 152, 1, [8, 8], [8, 8])
    monkeypatch.setenv("FACPPG_DECODER_SPLIT_MAX_NU", "4")
    assert shape(plan(DECODE, 10)) == (2, 4, 237, 1, [4, 4], [4, 4])
    monkeypatch.setenv("FACPPG_DECODER_SPLIT_MAX_NU", "9")   # the kernels serve 4 at most
    assert shape(plan(DECODE, 13)) == (1, 0, 195, 1, [20, 20], [20, 20])
    monkeypatch.delenv("FACPPG_DECODER_SPLIT_MAX_NU")
    monkeypatch.setenv("FACPPG_DECODER_NO_ROWS", "")
    monkeypatch.setenv("FACPPG_DECODER_PROF", "0")
    r = plan(DECODE, 1)
    assert (r.dbg_flags, r.prof) == (1, 1) and plan(FORCED, 1).prof == 1
    assert plan(DECODE, 10).dbg_flags == 0                   # a split launch's flag only


def test_decoder_step_qres_and_pause(monkeypatch):
    monkeypatch.setenv("FACPPG_DECODER_QRES", "1")
    r = plan(DECODE, 1)
    assert (r.q_res, r.lds_bytes) == (1, MAIN + 8192)
    monkeypatch.setenv("FACPPG_DECODER_QRES", "-5")
    assert plan(DECODE, 1).q_res == 0
    monkeypatch.setenv("FACPPG_DECODER_QRES", "100")
    assert plan(DECODE, 1).q_res == 3
    for text, want in (("300", 255), ("-3", 0), ("7", 7), ("0", 0)):
        monkeypatch.setenv("FACPPG_DECODER_PAUSE", text)
        assert plan(DECODE, 1).pause == want
    monkeypatch.delenv("FACPPG_DECODER_PAUSE")
    monkeypatch.setenv("FACPPG_DECODER_STEP", "legacy")
    r = plan(DECODE, 1)
    assert shape(r) == (2, 1, 76, 1, [4, 4], [4, 4]) and (r.step, r.q_res, r.pause, r.lds_bytes) == (2, 0, 0, MAIN)
    assert shape(plan(DECODE, 9)) == (2, 3, 234, 1, [4, 4], [4, 4])       # NU does not depend on the step
    assert plan(DECODE, 10).step == 0
    monkeypatch.setenv("FACPPG_DECODER_PAUSE", "5")
    assert plan(DECODE, 1).pause == 5
    monkeypatch.setenv("FACPPG_DECODER_STEP", "Legacy")      # any other text is the default
    assert plan(DECODE, 1).step == 1


def test_forced_follows_the_batch_and_the_bound():
    r = plan(FORCED, 2)
    assert (r.mode, r.step, r.regw, r.workgroups, r.launches) == (1, 0, 1, 226, 1) and list(r.first_u) == [4, 8]
    assert r.lds_bytes == MAIN
    r = plan(FORCED, 1)
    assert (r.regw, r.workgroups) == (1, 113)
    for B, u, wgs in ((3, [8, 8], 228), (4, [8, 20], 212), (6, [20, 20], 180), (8, [20, 20], 240), (16, [40, 75], 192), (60, [150, 150], 240)):
        r = plan(FORCED, B)
        assert (r.regw, r.workgroups, r.launches, list(r.first_u), list(r.last_u)) == (0, wgs, 1, u, u), B
    r = plan(FORCED, 61)
    assert (r.workgroups, r.launches, r.first_utts, r.last_utts, list(r.first_u), list(r.last_u)) == (76, 2, 60, 1, [150, 150], [8, 8])
    assert (plan(FORCED, 3, wgs=159).workgroups, list(plan(FORCED, 3, wgs=159).first_u)) == (159, [8, 20])
    r = plan(FORCED, 3, wgs=4)
    assert (r.workgroups, r.launches, r.first_utts, r.last_utts, list(r.last_u)) == (4, 3, 1, 1, [150, 150])
    r = plan(FORCED, 3, wgs=8)
    assert (r.workgroups, r.launches, r.first_utts, r.last_utts, list(r.first_u), list(r.last_u)) == (8, 2, 2, 1, [150, 150], [75, 75])
    plan(FORCED, 3, wgs=3, rc=EUNSUPPORTED)
    assert b"needs 4 co-resident workgroups, 3 allowed" in flib.load().facppg_last_error()
    plan(FORCED, 3, limit=0, rc=EUNSUPPORTED)


def test_forced_switches(monkeypatch):
    monkeypatch.setenv("FACPPG_FORCED_NO_REGW", "1")
    r = plan(FORCED, 2)
    assert (r.regw, r.workgroups, list(r.first_u)) == (0, 152, [8, 8])
    monkeypatch.delenv("FACPPG_FORCED_NO_REGW")
    for U in (8, 20, 40, 75, 150):
        monkeypatch.setenv("FACPPG_DECODER_COOP_U", str(U))
        r = plan(FORCED, 3)
        assert (r.regw, r.workgroups, list(r.first_u)) == (0, 3 * 2 * ((300 + U - 1) // U), [U, U])
    monkeypatch.setenv("FACPPG_DECODER_COOP_U", "20")
    assert plan(FORCED, 2).regw == 0                         # a forced width takes the register-resident chain away
    monkeypatch.setenv("FACPPG_DECODER_COOP_U", "8")
    plan(FORCED, 4, rc=EUNSUPPORTED)
    assert b"FACPPG_DECODER_COOP_U=8 does not fit B = 4" in flib.load().facppg_last_error()


def test_bilstm_follows_the_batch(monkeypatch):
    def kind(B, **kw):
        r = plan(ENCODE, B, **kw)
        assert (r.mode, r.launches) == (0, 1)
        return (r.bilstm_kind, r.bilstm_legacy, r.workgroups)
    for B in (1, 12):
        assert kind(B) == (1, 0, 10 * 2 * B)                 # 32 of 300 units per workgroup, two directions
    for B in (13, 24):
        assert kind(B) == (2, 0, 5 * 2 * B)
    assert kind(25) == (0, 0, 50) and kind(1, limit=0) == (0, 0, 2)
    assert kind(1, Tin=9000) == (1, 0, 20)                   # the encoder has no bound on Tin
    monkeypatch.setenv("FACPPG_BILSTM_STEP", "legacy")
    assert kind(12) == (1, 1, 240) and kind(13) == (2, 1, 130) and kind(25) == (0, 0, 50)
    monkeypatch.setenv("FACPPG_BILSTM_MODE", "wide")
    assert kind(1) == (2, 1, 10) and kind(25) == (0, 0, 50)
    monkeypatch.setenv("FACPPG_BILSTM_MODE", "single")
    assert kind(1) == (0, 0, 2)


def test_bad_arguments():
    plan(3, 1, rc=EINVAL)
    plan(DECODE, 0, rc=EINVAL)
    plan(DECODE, 1, Tin=0, rc=EINVAL)
    plan(DECODE, 1, steps=0, rc=EINVAL)
    plan(DECODE, 1, wgs=-1, rc=EINVAL)
    plan(DECODE, 1, limit=-1, rc=EINVAL)
    L = flib.load()
    assert L.facppg_taco_launch_plan(None, 240, DECODE, 1, 3, 4, 0, flib.TacoLaunchReport()) == EINVAL
    assert L.facppg_taco_launch_plan(reference_config(), 240, DECODE, 1, 3, 4, 0, None) == EINVAL
    assert L.facppg_taco_coop_limit(None) == 0


def test_planning_header_needs_no_hip(tmp_path):
    """csrc/facppg_taco_plan.h is plain host C++: it compiles on its own, with warnings as errors and no HIP include path."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "plan.cpp"
    src.write_text('#include "facppg_taco_plan.h"\n'
                   "int main() {\n"
                   "  using namespace facppg;\n"
                   "  facppg_taco_config c = {};\n"
                   "  c.prenet_dim = c.attention_rnn_dim = c.decoder_rnn_dim = 300; c.encoder_embedding_dim = 600;\n"
                   "  const TacoGeometry g = taco_geometry(c, 240);\n"
                   "  const TacoTuning t = taco_tuning_from_env();\n"
                   "  return plan_bilstm(g, 1, t).kind + plan_decode(g, 1, 3, 4, 0, false, t).rc + plan_forced(g, 1, 3, 0, t).rc;\n"
                   "}\n")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "fac-via-ppg_amd", "csrc"), str(src)])
