"""Batched PPG -> mel -> wav synthesis (BASELINE configs 3 and 4).

The reference synthesises one utterance at a time (generate_synthesis.py:90-95).  ``synthesize``
runs the same three stages -- Tacotron2.inference, WaveGlow.infer, Denoiser -- on a padded batch
with per-utterance lengths threaded through every HIP call, so each utterance's result equals
its own batch-1 run; everything stays on the device until the final copy of the audio.
"""
import os
import threading

import numpy as np
import torch


class Synthesizer(object):
    """The three models of the synthesis path loaded from the reference's checkpoint formats and kept on the GPU:
    the PPG->mel state dict (``{'state_dict': ...}``, train_ppg2mel.py:113-119), the pickled WaveGlow module
    (``{'model': ...}``, train_waveglow.py:56-64) once with weight norm removed for synthesis
    (utils.py:177-181) and once as pickled for the denoiser's bias estimate (generate_synthesis.py:58-61)."""

    def __init__(self, ppg2mel_path, waveglow_path, hparams=None, denoiser_mode='zeros', vocoder_arithmetic=None, vocoder_stream=None):
        """waveglow_path None: a synthesizer without a vocoder (none trained yet for this speaker) -- it has the PPG -> mel model
        and the hparams' TacotronSTFT, and offers preview / preview_wavs / preview_scored (Griffin-Lim on the device); every
        method that needs the vocoder raises."""
        from common.hparams import create_hparams_stage
        from common.layers import TacotronSTFT
        from script.train_ppg2mel import load_model
        self.hparams = hparams if hparams is not None else create_hparams_stage()
        hp = self.hparams
        self.tacotron = load_model(hp)
        self.tacotron.load_state_dict(torch.load(ppg2mel_path, weights_only=False)['state_dict'])
        self.tacotron.eval()
        # the analysis the model's mels were made with (common.data_utils.PPGMelLoader): what preview inverts
        self.stft = TacotronSTFT(hp.filter_length, hp.hop_length, hp.win_length, hp.n_acoustic_feat_dims, hp.sampling_rate,
                                 hp.mel_fmin, hp.mel_fmax)
        self.stft.to(next(self.tacotron.parameters()).device)
        self.denoiser = self.waveglow = None
        self.vocoder_less = waveglow_path is None
        if waveglow_path is not None:
            from common.utils import load_waveglow_model
            from waveglow.denoiser import Denoiser
            self.denoiser = Denoiser(torch.load(waveglow_path, weights_only=False)['model'].cuda(), mode=denoiser_mode)
            self.waveglow = load_waveglow_model(waveglow_path)
        # the vocoder's arithmetic of every call (WaveGlow.infer's ``arithmetic``); the denoiser's bias spectrum above is formed on
        # the fp32 path either way
        self.vocoder_arithmetic = _checked_arithmetic(vocoder_arithmetic)
        # synthesize()'s ``vocoder_stream`` of every one-utterance call (True: a "bf16x3" vocoder takes the streamed, conditioning-first path)
        self.vocoder_stream = _checked_stream(vocoder_stream)

    def _vocoder(self, what):
        """Refuses ``what`` on a synthesizer built without a vocoder, before any device work."""
        if getattr(self, "vocoder_less", False):
            from facppg.lib import FacppgError
            raise FacppgError("Synthesizer.%s needs the vocoder, and this synthesizer was built without one (waveglow_path=None): "
                              "use preview / preview_wavs / preview_scored, which make the waveform by Griffin-Lim" % what)

    def __call__(self, ppgs, sigma=0.6, strength=0.005, **kw):
        self._vocoder("__call__")
        kw.setdefault("vocoder_arithmetic", self.vocoder_arithmetic)
        kw.setdefault("vocoder_stream", self.vocoder_stream)
        return synthesize(ppgs, self.tacotron, self.waveglow, self.denoiser, sigma=sigma, strength=strength, **kw)

    def stream(self, jobs, sigma=0.6, strength=0.005, **kw):
        """synthesize_stream over this synthesizer's models: batch i+1's acoustic model under batch i's vocoder.  Jobs that carry
        ``wavs`` need ``ppg_deps`` (a ppg.DependenciesPPG)."""
        self._vocoder("stream")
        kw.setdefault("vocoder_arithmetic", self.vocoder_arithmetic)
        return synthesize_stream(jobs, self.tacotron, self.waveglow, self.denoiser, sigma=sigma, strength=strength, **kw)

    def preview(self, ppgs, **kw):
        """facppg.pipeline.preview over this synthesizer's PPG -> mel model and TacotronSTFT: PPGs -> (waveforms, mel lengths)
        without a vocoder.  Works with or without one loaded."""
        return preview(ppgs, self.tacotron, self.stft, **kw)

    def preview_wavs(self, wavs, ppg_deps=None, **kw):
        """facppg.pipeline.preview_wavs over this synthesizer's models: teacher wavs (list of WaveData) -> (waveforms, mel
        lengths), the PPGs kept on the device; ppg_deps as in convert()."""
        _checked_wav_list(wavs, kw.get("ppgs"), "Synthesizer.preview_wavs")
        return preview_wavs(wavs, self._deps(ppg_deps), self.tacotron, self.stft, **kw)

    def preview_scored(self, wavs, ppg_deps=None, score_band=0, phones=False, **kw):
        """preview_wavs() plus facppg.score.roundtrip of what it made, in convert_scored's return shape: (waveforms, mel lengths,
        scores).  The waveforms are preview_wavs()'s for the same keywords, bit for bit."""
        from facppg import score
        _checked_wav_list(wavs, kw.get("ppgs"), "Synthesizer.preview_scored")
        deps = self._deps(ppg_deps)
        score.check_roundtrip_deps(deps, "Synthesizer.preview_scored")
        host = not kw.pop("return_device", False)
        audio, tout = self.preview_wavs(wavs, deps, return_device=True, **kw)
        scores = score.roundtrip(wavs, audio, self.hparams.sampling_rate, deps, band=score_band, phones=phones)
        if host:
            audio = [a.cpu().numpy() for a in audio]
        return audio, tout, scores

    def _deps(self, ppg_deps):
        """The PPG dependencies of a call that starts from audio: the caller's, else ppg.DependenciesPPG() read once."""
        if ppg_deps is not None:
            return ppg_deps
        if getattr(self, "ppg_deps", None) is None:
            from ppg import DependenciesPPG
            self.ppg_deps = DependenciesPPG()
        return self.ppg_deps

    def convert(self, wavs, ppg_deps=None, sigma=0.6, strength=0.005, ppgs=None, **kw):
        """synthesize_wavs over this synthesizer's models: teacher wavs (list of WaveData) -> (waveforms, mel lengths); the PPGs
        go from the front end to the encoder on the device.  ppg_deps: a ppg.DependenciesPPG (None: the default files, which
        are read only for a well-formed list of wavs)."""
        self._vocoder("convert")
        _checked_wav_list(wavs, ppgs, "Synthesizer.convert")
        kw.setdefault("vocoder_arithmetic", self.vocoder_arithmetic)
        kw.setdefault("vocoder_stream", self.vocoder_stream)
        return synthesize_wavs(wavs, self._deps(ppg_deps), self.tacotron, self.waveglow, self.denoiser, sigma=sigma, strength=strength, **kw)

    def convert_scored(self, wavs, ppg_deps=None, score_band=0, phones=False, **kw):
        """convert() plus facppg.score.roundtrip of what it made: (waveforms, mel lengths, scores).  The waveforms are convert()'s
        for the same keywords, bit for bit; the scores are roundtrip(wavs, waveforms, hparams.sampling_rate, ppg_deps,
        band=score_band, phones=phones) -- the converted audio goes back through the front end next to the teacher's and the two
        monophone PPGs are aligned on the device; with ``phones`` the scores also say per teacher phone where it landed
        (facppg.align.phone_report).  Dependencies without the pdf -> monophone matrix are refused before anything runs."""
        from facppg import score
        self._vocoder("convert_scored")
        _checked_wav_list(wavs, kw.get("ppgs"), "Synthesizer.convert_scored")
        deps = self._deps(ppg_deps)
        score.check_roundtrip_deps(deps, "Synthesizer.convert_scored")
        host = not kw.pop("return_device", False)
        audio, tout = self.convert(wavs, deps, return_device=True, **kw)
        scores = score.roundtrip(wavs, audio, self.hparams.sampling_rate, deps, band=score_band, phones=phones)
        if host:
            audio = [a.cpu().numpy() for a in audio]
        return audio, tout, scores

    def convert_file(self, utterance_path, wav_path, fs, sigma=0.6, strength=0.005, ppg_deps=None):
        """synthesize_file from the teacher wav itself: ``utterance_path`` (a wav) -> ``wav_path`` (float32 [N, 1] at ``fs``,
        generate_synthesis.py:86-98), the PPGs extracted here and kept on the device."""
        from common.feat import read_wav_kaldi
        from scipy.io import wavfile
        self._vocoder("convert_file")
        wavs, tout = self.convert([read_wav_kaldi(utterance_path)], ppg_deps, sigma=sigma, strength=strength)
        wavfile.write(wav_path, fs, wavs[0].astype(np.float32)[:, None])
        return tout[0]

    def convert_long(self, wavs, ppg_deps=None, **kw):
        """synthesize_long_wavs over this synthesizer's models: teacher recordings of any length (list of WaveData) ->
        (waveforms, segment tables), cut at their pauses, converted in batches and joined on the device.  Keywords and defaults
        are synthesize_long_wavs's (the vocoder arithmetic defaults to the synthesizer's); ppg_deps as in convert()."""
        self._vocoder("convert_long")
        _checked_wav_list(wavs, None, "Synthesizer.convert_long")
        kw.setdefault("vocoder_arithmetic", self.vocoder_arithmetic)
        return synthesize_long_wavs(wavs, self._deps(ppg_deps), self.tacotron, self.waveglow, self.denoiser, **kw)

    def convert_long_file(self, utterance_path, wav_path, fs, **kw):
        """convert_file for a recording of any length (convert_file itself stops at max_decoder_steps frames, as the reference
        does): ``utterance_path`` (a wav) -> ``wav_path`` (float32 [N, 1] at ``fs``).  Returns the recording's segment table."""
        from common.feat import read_wav_kaldi
        from scipy.io import wavfile
        self._vocoder("convert_long_file")
        kw["return_device"] = False
        wavs, tables = self.convert_long([read_wav_kaldi(utterance_path)], **kw)
        wavfile.write(wav_path, fs, wavs[0].astype(np.float32)[:, None])
        return tables[0]

    @staticmethod
    def has_utterance(utterance_path):
        """The reference checks the teacher wav itself (generate_synthesis.py:89); here a precomputed PPG next to
        it (or given directly) counts as well, since that is what this build reads."""
        from common.data_utils import ppg_candidates
        return any(os.path.isfile(c) for c in [utterance_path] + ppg_candidates(utterance_path))

    def synthesize_file(self, utterance_path, wav_path, fs, sigma=0.6, strength=0.005, ppg_deps=None):
        """One teacher utterance -> ``wav_path`` (float32 [N, 1] at ``fs``, generate_synthesis.py:90-98)."""
        from common.data_utils import get_ppg
        from scipy.io import wavfile
        self._vocoder("synthesize_file")
        wavs, tout = self([get_ppg(utterance_path, ppg_deps)], sigma=sigma, strength=strength)
        wavfile.write(wav_path, fs, wavs[0].astype(np.float32)[:, None])
        return tout[0]


class ConditioningStream(object):
    """One utterance at a time (the metric's "batch = 1" case): work that depends on the mel frames ALONE, done while the decoder
    is still producing them, on the ~180 CUs its launch leaves empty.

    The split decoder publishes every frame the moment it exists (facppg_taco_decode_opts); on a second HIP stream, gated
    on those frames (facppg_taco_collect_frames), this object runs per block of frames
      * the postnet as a streaming convolution stack (facppg_taco_postnet_range: same sums, same order, same bits as the one-shot
        launch) straight into the vocoder's zero-margined mel buffer, and
      * the conditioning part of every WaveNet layer's gate GEMM (facppg_wg_cond_seed: bias + the folded conditioning chunks, the
        MFMA sequence the layer kernel itself would run first) into a seed buffer,
    so that behind the decoder only the last frames' share is left, and WaveGlow's layer launches start from the seeds with 12 K
    chunks instead of 17 (first layers 1 instead of 6): 29 % of the vocoder's FLOPs off the critical path, same samples bit for
    bit (tests/test_gpu_stream.py).  Reference: Postnet.forward (model.py:178-184, 604-605), WN.forward's cond_layers
    (glow.py:154-175) and the upsampling they read (glow.py:253-259).

    A pass over a block of frames streams every (flow, layer, phase) conditioning image once -- 2 GB at hop 256 -- whatever the
    block's width (FACPPG_STREAM_CHUNK frames: 32 for utterances up to 320 frames, 64 beyond, the last one before the expected
    end always 32, which keeps the share that has to wait for the decoder's end small).  What the blocks cannot cover -- the frames
    that become final only when the decoder ends -- runs as UNSEEDED 16-frame tiles inside the vocoder's own layer launches
    (k_wn_layer_mixed) or gets its seeds from one more pass in front of them: tail_pass() decides.

    A .half() vocoder (the reference's inference.py --is_fp16 recipe) streams the same way on the fp16 kernels: every block's
    postnet columns are rounded into the vocoder's fp16 mel buffer behind the postnet (facppg_wg_mel_pad_f16), the seed passes are
    k16_cond_seed's (raw fp32 conditioning sums, 1.0 GB of fp16 images per pass), the layer launches run conditioning-first
    (facppg_wg_infer_seeded_f16), and the tail tiles get their seeds from one more pass behind the decoder.  Bit for bit the
    samples of the unstreamed pipeline, which runs a half vocoder conditioning-first for one utterance too
    (tests/test_gpu_stream_f16.py).

    The split-bf16 arithmetic of an fp32 vocoder (synthesize(vocoder_arithmetic="bf16x3", vocoder_stream=True): opt-in per call) is
    the third kind and streams like the fp16 one: every block's postnet columns are copied into the split path's fp32 [Tqp][80] mel
    buffer behind the postnet (facppg_wg_split_mel_pad), the seed passes are ks_cond_seed's on the split handle (raw fp32 sums of the
    split products, 2.0 GB of hi / lo images per pass, block_tiles clamped to what the LDS holds), the layer launches run
    conditioning-first (facppg_wg_split_infer_seeded) and the tail tiles get their seeds from one more pass behind the decoder.  Bit
    for bit the samples of the unstreamed opt-in call (mel_pad + infer_seeded with no seeded frame; tests/test_gpu_stream_bf16x3.py);
    in the last bits NOT those of the plain vocoder_arithmetic="bf16x3" call, which sums the taps first and never comes here.  One
    model pair may serve utterances of its precision's kind and of this one alternately: the buffers are re-laid-out per kind.

    Host flow of one utterance: begin() (kind, layout, zeroed frame words) -> enqueue() (per planned block: _mel_block on
    the postnet stream, _seed_pass on the seed stream) -> finish() (_mel_block for the frames behind the last block) -> vocode()
    (tail_pass, possibly one more _seed_pass, WaveGlow.infer_seeded)."""

    def __init__(self, tacotron, waveglow):
        self.tacotron, self.waveglow = tacotron, waveglow
        self.key = None            # the device the side streams and ``store`` belong to
        self.store = {}            # the allocations behind every buffer view: grow only, re-used by every utterance
        self.layout_key = self.layout = None
        self.active = False
        self.profile = False       # True: hipEvents around every seed pass of the following utterances (pass_ms)
        self.lock = threading.Lock()   # held by synthesize() for the whole utterance (buffers, streams and plan are per model pair)
        # per utterance: set by begin() (dtype, half, cap), enqueue() (cuts, the events, n_launch), finish() (Tout, seeded, void_blocks)
        self.dtype, self.half, self.split, self.cap, self.lag = None, False, False, 0, None
        self.melp16 = self.melp_split = None
        self.max_block_tiles = 4
        self.dev = self.steps = self.Tin = self.taco_handle = self.wg_handle = None
        self.cuts, self.n_extra, self.n_launch = [], 0, 0
        self.last_final, self.finals, self.flow_events, self.pass_events = None, [], {}, []
        self.Tout = self.seeded = self.void_blocks = 0

    @staticmethod
    def _switched_on(tacotron, waveglow):
        if os.environ.get("FACPPG_STREAM", "1") == "0" or os.environ.get("FACPPG_WG_UNFOLDED", "0") not in ("", "0"):
            return False
        if os.environ.get("FACPPG_WG_EDGE_FOLD", "1") == "0" or getattr(tacotron, "decoder_workgroups", 0):
            return False
        return waveglow.WN[0].n_layers == 8 and waveglow.n_group == 8

    @staticmethod
    def usable(tacotron, waveglow):
        """The streamed path exists for the reference's shapes on the folded, phase-major vocoder kernels, all fp32 or all fp16 (the
        reference's .half() recipe): bf16 and mixed modules run unstreamed (or are refused).  An all-fp32 vocoder streams its own
        arithmetic and, for the calls that opt in, the split-bf16 one (begin() is told which)."""
        return ConditioningStream._switched_on(tacotron, waveglow) and ConditioningStream.precision(waveglow) is not None

    @staticmethod
    def precision(waveglow, walk=True):
        """torch.float32 / torch.float16: the kernels the stream would feed; None: neither (bf16, mixed dtypes).  walk=False takes
        the upsampler's word for a half vocoder (callers whose next step, WaveGlow.infer, refuses a mixed module itself)."""
        dt = getattr(getattr(waveglow, "upsample", None), "weight", torch.empty(0)).dtype
        if dt == torch.float16 and walk:      # every WN / upsample parameter must be (the walk is spent on half vocoders only)
            if hasattr(waveglow, "_precision"):
                from facppg.lib import FacppgError
                try:
                    return dt if waveglow._precision() == dt else None
                except FacppgError:
                    return None
            dts = {p.dtype for p in waveglow.upsample.parameters()} | {p.dtype for wn in waveglow.WN for p in wn.parameters()}
            return dt if dts == {dt} else None
        return dt if dt in (torch.float32, torch.float16) else None

    # Utterances shorter than this are not streamed (FACPPG_STREAM_MIN_FRAMES overrides), per vocoder precision.  fp32: see begin().
    # fp16: streamed wins at every length of the sweep (64 frames 5.8 -> 5.3 ms, 100: 6.7 -> 6.3, 130: 7.4 -> 7.0, 200: 9.2 -> 8.8,
    # 400: 16.1 -> 15.2; profiles/r11_stream_f16_sweep.txt) -- its layer launches are 32-frame tiles streamed or not, so a seeded
    # launch is shorter at any length; 64 frames is the shortest utterance the sweep covers.
    MIN_FRAMES = {torch.float32: 128, torch.float16: 64}
    # The split-bf16 kind (opt-in calls): like fp16, its layer launches are 32-frame tiles streamed or not, so a seeded launch is
    # shorter at any length; the figure is the shortest length of the sweep from which streamed wins at every longer one
    # (profiles/r16_stream_split_sweep.txt: 64 frames 7.08 -> 5.76 ms, 100: 7.95 -> 6.64, 130: 8.82 -> 7.50, 200: 10.97 -> 9.44,
    # 400: 19.18 -> 17.07, 1000: 41.32 -> 36.97).
    MIN_FRAMES_SPLIT = 64
    SPLIT = "bf16x3"   # the kind's name: WaveGlow's ``arithmetic``, tail_pass()'s ``precision``

    SLACK = 64   # frames past the PPG's length the buffers are laid out for (an utterance that runs on past them is finished unstreamed)

    def _buffers(self, dev, steps, cap):
        """Views for one utterance: the frame words cover the decoder's step limit ``steps`` (it publishes every frame it makes), the
        vocoder-side buffers (zero-margined mel, seeds, the streaming postnet's layers) are LAID OUT for ``cap`` <= steps frames --
        the PPG's length plus SLACK, not max_decoder_steps: 64 KiB of seeds per (layer, phase, 32 frames) is 1.9 GB at 288 frames and
        6.4 GB at 1000.  The allocations only ever grow (an utterance of another length re-uses them under its own layout) and the
        two side streams are created once per device."""
        from facppg import lib as _lib
        L = _lib.load()
        hp = self.tacotron._hp
        self.NF = hp["n_acoustic_feat_dims"]
        self.lag = (hp["postnet_kernel_size"] - 1) // 2 * hp["postnet_n_convolutions"]
        if self.key != dev:
            self.store = {}
            # The seed passes fill every CU the decoder leaves; the postnet's launches next to them are a few workgroups each and must
            # not queue for a slot behind thousands of the pass's own (measured: 260 us for a 22 us launch): the seed stream gets the
            # lowest priority, the postnet stream the highest (FACPPG_STREAM_PRIO=0: both default).
            lo, hi = torch.cuda.Stream.priority_range() if hasattr(torch.cuda.Stream, "priority_range") else (0, 0)
            if os.environ.get("FACPPG_STREAM_PRIO", "1") == "0":
                lo = hi = 0
            self.side = torch.cuda.Stream(device=dev, priority=max(lo, hi))          # the seed passes (largest number = lowest priority)
            # frame collection + the streaming postnet, one block ahead of them (FACPPG_STREAM_ONE=1: on the same stream, experiments)
            self.post = self.side if os.environ.get("FACPPG_STREAM_ONE") == "1" else torch.cuda.Stream(device=dev, priority=min(lo, hi))
            self.prio = (lo, hi)
            self.key = dev

        def grown(name, numel, dtype, zero=False):
            t = self.store.get(name)
            if t is None or t.numel() < numel:
                self.store[name] = t = (torch.zeros if zero else torch.empty)(numel, dtype=dtype, device=dev)
            return t[:numel]
        # (the layout queries validate the models' packed-weight handles -- ~1000 tensors, 0.2 - 0.4 ms of host time in front of the
        #  encoder: asked once per (step limit, layout), not per utterance)
        lk = (dev, steps, cap, self.half, self.split)
        if self.layout_key != lk:
            lay = self.waveglow.seed_layout(cap, dev, block_tiles=True, **self._kind())
            self.layout = lay + (L.facppg_taco_postnet_stream_workspace_bytes(self.tacotron._handle(dev), cap),)
            self.layout_key = lk
        self.tqp, self.margin, seed_bytes, self.max_block_tiles, post_ws_bytes = self.layout
        # {value, frame + 1} words + the void flags + the work counters + mel_post in the vocoder's zero-margined layout: ONE allocation,
        # zeroed by one launch before every decode
        # (a half vocoder: + the same frames in ITS layout, fp16 [tqp][NF], converted block by block behind the postnet; the split
        #  kind: + the same in fp32 [tqp][NF])
        nw = steps * self.NF + 512
        n32 = (self.NF * self.tqp + 1) // 2
        n16 = (self.NF * self.tqp + 3) // 4 if self.half else n32 if self.split else 0
        self.zeroed = grown("zeroed", nw + n32 + n16, torch.int64, zero=True)
        self.melp16 = self.zeroed[nw + n32:nw + n32 + n16].view(torch.float16)[:self.NF * self.tqp].view(self.tqp, self.NF) if self.half else None
        self.melp_split = self.zeroed[nw + n32:nw + n32 + n16].view(torch.float32)[:self.NF * self.tqp].view(self.tqp, self.NF) if self.split else None
        self.words = self.zeroed[:nw]
        self.void = self.words[steps * self.NF:].view(torch.int32)[:512]                  # one per block
        self.counters = self.words[steps * self.NF:].view(torch.int32)[512:]              # one per bounded seed launch
        self.melp = self.zeroed[nw:nw + n32].view(torch.float32)[:self.NF * self.tqp].view(self.NF, self.tqp)
        self.mel = grown("mel", self.NF * steps, torch.float32, zero=True).view(self.NF, steps)   # collected frames, channel-major
        if "void_host" not in self.store:
            self.store["void_host"] = torch.zeros(512, dtype=torch.int32).pin_memory()
        self.void_host = self.store["void_host"]
        self.seeds = grown("seeds", seed_bytes // 4, torch.float32)
        self.post_ws = grown("post_ws", post_ws_bytes, torch.uint8)

    def footprint_bytes(self):
        """Device memory the stream holds on to between utterances."""
        return sum(t.numel() * t.element_size() for t in self.store.values() if t.is_cuda)

    def plan(self, steps, Tin):
        """[(frames of mel needed, first seeded frame, end of seeded frames)] -- blocks that can be formed before the utterance ends
        if it runs to about min(steps, Tin) frames; whatever is not covered is left for finish().  Reads ``lag`` and ``cap`` (the
        frames the vocoder-side buffers are laid out for), leaves ``n_extra``."""
        end = min(steps, max(Tin, 1))
        # 32-frame blocks keep every block's postnet chain clear of the previous block's pass (a block every 0.62 ms, chain + pass
        # 0.6 ms) at 2 GB of weight images per block; utterances of several seconds take 64-frame blocks (half the HBM traffic
        # next to the decoder) except for the last one before the expected end
        chunk = max(32, int(os.environ.get("FACPPG_STREAM_CHUNK", "32" if end <= 320 else "64")) // 32 * 32)
        last = max(32, int(os.environ.get("FACPPG_STREAM_LAST", "32")) // 32 * 32)
        s_end = (end - self.lag) // 32 * 32                       # seeded frames before the expected end
        cuts, s = [], 0
        widths = [int(v) // 32 * 32 for v in os.environ.get("FACPPG_STREAM_PLAN", "").split(",") if v.strip()]   # (experiments)
        while s < s_end and len(cuts) < 120:
            rest = s_end - s
            w = rest if rest <= last else min(chunk, rest - last)
            if widths:
                w = max(32, min(widths.pop(0), rest))
            cuts.append((s + w + self.lag, s, s + w))
            s += w
        s_lim = (min(steps, self.cap) - self.lag) // 32 * 32   # the decoder may run on towards its step limit: a few more blocks (inside the layout)
        extra = 0
        while s < s_lim and extra < 2 and len(cuts) < 120:
            w = min(chunk, s_lim - s)
            cuts.append((s + w + self.lag, s, s + w))
            s += w
            extra += 1
        self.n_extra = extra
        return cuts

    # ---- called by Tacotron2.inference
    def begin(self, tacotron, handle, dev, steps, Tin, arithmetic=None):
        """Before the decoder launch, on its stream: zeroed frame words.  Returns them (None: not usable for this call).
        arithmetic: the vocoder arithmetic of THIS utterance -- None: the module's own (fp32 / fp16 kind); "bf16x3": the split kind."""
        self.active = False
        # Short utterances do not gain: up to 128 frames the unstreamed vocoder runs 16-frame tiles, one per CU, and a layer launch
        # lasts as long as ONE tile either way (measured, tools/stream_T_sweep.sh: 64 frames 6.9 -> 8.1 ms, 100 frames 8.2 -> 9.0
        # streamed; 130 frames 10.0 -> 9.7, 200 frames 13.3 -> 11.5, 1000 frames 53.9 -> 48.5).  FACPPG_STREAM_MIN_FRAMES overrides.
        self.dtype = self.precision(self.waveglow) if self._switched_on(tacotron, self.waveglow) else None    # (usable(), keeping the answer)
        if self.dtype is None:
            return None
        self.half = self.dtype == torch.float16
        self.split = arithmetic == self.SPLIT
        if self.split and self.dtype != torch.float32:       # (split operands are an fp32 module's: the vocoder stage refuses the rest)
            return None
        if min(steps, Tin) < int(os.environ.get("FACPPG_STREAM_MIN_FRAMES", self.MIN_FRAMES_SPLIT if self.split else self.MIN_FRAMES[self.dtype])):
            return None
        self.cap = min(steps, -(-(Tin + self.SLACK) // 32) * 32)
        try:
            self._buffers(dev, steps, self.cap)
        except torch.cuda.OutOfMemoryError:                 # (no room for the seeds next to whatever else lives here: run unstreamed)
            self.key, self.store = None, {}
            return None
        self.dev, self.steps, self.Tin, self.taco_handle = dev, steps, Tin, handle
        cur = torch.cuda.current_stream(dev)
        cur.wait_stream(self.side)      # (an utterance that was abandoned half way -- an exception between the decoder and the vocoder --
        cur.wait_stream(self.post)      #  may have left launches behind on the side streams: they read the buffers zeroed next)
        self.zeroed.zero_()
        self.ready = torch.cuda.Event()
        self.ready.record(torch.cuda.current_stream(dev))
        return self.words

    def cancel(self):
        self.active = False

    def enqueue(self, out_len, decoder_workgroups):
        """The decoder has been launched (on ``decoder_workgroups`` CUs) and publishes its frames: enqueue every planned block on
        the side stream."""
        dev = self.dev
        self.cuts = self.plan(self.steps, self.Tin)
        self.wg_handle = self.waveglow.handle(dev, **self._kind())
        f_prev = 0
        lpw = max(1, int(os.environ.get("FACPPG_STREAM_LPW", "1")))
        # The seed passes take the CUs the decoder leaves except `spare` of them, ONE workgroup per CU that holds the CU's whole LDS
        # (a bounded launch does, see facppg_wg_cond_seed): the dispatcher otherwise places the postnet's small workgroups -- and the
        # first launches behind the decoder on the main stream -- next to a pass's workgroups, where they crawl (3-5x, measured).
        n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
        spare = int(os.environ.get("FACPPG_STREAM_SPARE_CUS", "8"))
        bound = max(16, n_cu - decoder_workgroups - spare) if spare >= 0 else 0
        self.n_launch = 0
        self.last_final, self.finals, self.flow_events, self.pass_events = None, [], {}, []
        self.post.wait_event(self.ready)
        for k, (f_new, s_a, s_b) in enumerate(self.cuts):
            void = self.void[k:k + 1]
            with torch.cuda.stream(self.post):
                self._mel_block(out_len, f_prev, f_new, void=void, void_before=self.void[k - 1:k] if k else None)
                # (the block's void flag travels to pinned host memory behind its collector, on this stream: when the decoder has
                #  ended the flags of the blocks it covered have been on the host for milliseconds -- finish() reads them there
                #  instead of spending a second device->host round trip between the decoder and the vocoder)
                self.void_host[k:k + 1].copy_(void, non_blocking=True)
                final = torch.cuda.Event()
                final.record(self.post)
                self.last_final = final
                self.finals.append(final)
            with torch.cuda.stream(self.side):
                self.side.wait_event(final)                # mel_post is final up to s_b
                self._seed_pass(s_a, s_b - s_a, min(4, (s_b - s_a) // 32), lpw, bound, skip=void, timed=self.profile)
                ev = torch.cuda.Event()
                ev.record(self.side)
                self.flow_events = {self.waveglow.n_flows - 1: ev}   # the vocoder's first launches (last flow) wait for the last pass
            f_prev = f_new
        self.active = True

    def _mel_block(self, out_len, f0, f1, Tout=0, void=None, void_before=None):
        """Decoder frames [f0, f1) on the current stream: collected, through the streaming postnet into the vocoder's mel buffer, and
        the postnet columns they make final rounded into a half vocoder's.  Tout (finish(): f1 is the utterance's end) makes every
        column up to f1 final; under the decoder the postnet trails by ``lag`` frames.  void / void_before: the block's flag and the
        flag of the block in front of it (a block whose frames do not arrive in time raises its flag and writes nothing)."""
        from facppg import lib as _lib
        L = _lib.load()
        with torch.cuda.device(self.dev):
            st = _lib.current_stream(self.dev)
            if f1 > f0:
                _lib.check(L.facppg_taco_collect_frames(self.taco_handle, _lib.ptr(self.words), _lib.ptr(out_len), f0, f1,
                                                        _lib.ptr(self.mel), self.steps, _lib.ptr(void), _lib.ptr(void_before), st))
            _lib.check(L.facppg_taco_postnet_range(self.taco_handle, _lib.ptr(self.mel), self.steps, f0, f1, Tout,
                                                   self.melp.data_ptr() + 4 * self.margin, self.tqp, _lib.ptr(self.post_ws),
                                                   self.post_ws.numel(), self.cap, _lib.ptr(void), st))
        if self.half or self.split:
            c0 = max(0, f0 - self.lag)
            self.waveglow.mel_convert(self.melp[:, self.margin:], self.cap, c0, (f1 if Tout else f1 - self.lag) - c0,
                                      self.melp_split if self.split else self.melp16, skip=void, handle=self.wg_handle, **self._kind())

    def _kind(self):
        """The keyword that sends a WaveGlow seeded method to this utterance's kernels."""
        return {"arithmetic": self.SPLIT} if self.split else {}

    def _vocoder_mel(self):
        return self.melp_split if self.split else self.melp16 if self.half else self.melp

    def _seed_pass(self, frame0, nframes, block_tiles, layers_per_workgroup, max_workgroups, skip=None, timed=False):
        """One k_cond_seed launch over frames [frame0, frame0 + nframes), every flow, on the current stream (block_tiles clamped to
        what the kind's seed kernel takes).  max_workgroups None:
        an unbounded launch; otherwise (0 included: the bound may come from the environment) the launch takes the utterance's next
        zeroed work counter, and runs unbounded once the counters are used up.  timed: hipEvents around it for pass_ms()."""
        counter = None
        if max_workgroups is not None:
            if self.n_launch < 500:
                counter = self.counters[self.n_launch:self.n_launch + 1]
            else:
                max_workgroups = 0
            self.n_launch += 1
        if timed:
            stream = torch.cuda.current_stream(self.dev)
            e0 = torch.cuda.Event(enable_timing=True)
            e0.record(stream)
        self.waveglow.cond_seed(self._vocoder_mel(), self.cap, frame0, nframes, self.seeds, block_tiles=min(block_tiles, self.max_block_tiles),
                                layers_per_workgroup=layers_per_workgroup, skip=skip, handle=self.wg_handle,
                                max_workgroups=max_workgroups or 0, counter=counter, **self._kind())
        if timed:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record(stream)
            self.pass_events.append((nframes, self.waveglow.n_flows, e0, e1))

    def finish(self, Tout, out_len):
        """The decoder has ended at Tout frames (known on the host): what the blocks could not cover, on the caller's stream.
        Returns mel_post [1, NF, Tout] (a view of the vocoder's mel buffer, valid until the next streamed utterance on these models),
        or None when the utterance outgrew the stream's layout: the caller then runs the one-shot postnet and the ordinary vocoder."""
        cur = torch.cuda.current_stream(self.dev)
        if Tout > self.cap:       # the decoder ran on past the frames the buffers were laid out for (PPG length + SLACK): unstreamed
            cur.wait_stream(self.post)
            cur.wait_stream(self.side)
            self.active = False
            return None
        # what is left of the postnet needs the postnet stream's blocks only; the seed passes' events gate the vocoder's flows (vocode)
        if self.last_final is not None:
            cur.wait_event(self.last_final)
        # Which blocks were really formed: a block the decoder stopped short of is void (f_new > Tout, known from the length), but
        # so is a block whose frames did not arrive within FACPPG_STREAM_WAIT_MS (k_collect_frames gave up: a profiler serialising
        # kernels, cooperative launches queued behind another process) -- its postnet columns and seeds were never written, and
        # every block behind it is void too.  The flags are read back here (the blocks up to the decoder's end finished
        # milliseconds ago; the ones past it return the moment they see the length) and the tail below starts at the first void one.
        n_cov = sum(1 for f_new, _, _ in self.cuts if f_new <= Tout)
        self.void_blocks = 0
        if n_cov:
            self.finals[n_cov - 1].synchronize()          # (block k's flag is copied to the host ahead of its event)
            first_void = next((k for k in range(n_cov) if int(self.void_host[k])), n_cov)
            self.void_blocks, n_cov = n_cov - first_void, first_void
        f_done, _, s_done = self.cuts[n_cov - 1] if n_cov else (0, 0, 0)
        self._mel_block(out_len, f_done, Tout, Tout=Tout)
        self.Tout, self.seeded = Tout, s_done
        return self.melp[:, self.margin:self.margin + Tout].unsqueeze(0)

    def pass_ms(self):
        """[(frames, flows, ms)] of the seed passes of the most recent utterance (profile = True); synchronises them."""
        out = []
        for n, nf, e0, e1 in self.pass_events:
            e1.synchronize()
            out.append((n, nf, e0.elapsed_time(e1)))
        return out

    # ---- called by the vocoder stage
    @staticmethod
    def tail_pass(precision, T, seeded, P, n_cu, tail=None):
        """How the frames behind the last block -- [seeded, T) -- get their conditioning sums: None = inside the vocoder's layer
        launches, as unseeded tiles (or nothing is left); otherwise the seed pass to run in front of the vocoder, (first frame,
        frames, block_tiles, layers_per_workgroup, bounded).  P: phases (hop / 8); n_cu: CUs of the device; tail: the value of
        FACPPG_STREAM_TAIL ("seed" / "mixed" force either side; default fp32 "auto", fp16 "seed").

        fp32: unseeded 16-frame tiles inside the layer launches (k_wn_layer_mixed) while the mixed launch needs no more ROUNDS of one
        workgroup per CU than the all-seeded one would (measured: 230 frames, 288 against 256 workgroups: 17.5 against 13.4 ms per
        step; 300 / 350 / 450 frames, two rounds either way: the mixed launch is 0.35 - 0.85 ms ahead of the extra pass); needs
        seeded tiles in front (0 < seeded < T).
        fp16: seeded and unseeded tiles of the fp16 launches are both 32 frames wide, so a launch with ONE unseeded tile lasts as long
        as an unseeded launch (every tile has a CU of its own at these lengths): one more pass, one workgroup per CU walking the
        work items from a counter -- the pass streams the images fastest that way (200 frames, two tail tiles: 8.8 ms against
        9.1 ms end to end with the in-kernel tail, profiles/r11_stream_f16_ab.txt).  Same samples either way.
        "bf16x3" (the split kind): fp16's rule for fp16's reason -- seeded and unseeded tiles are both 32 frames wide (the block
        width is clamped to the kernel's by _seed_pass; both variants at 200 frames: profiles/r16_stream_split_ab.txt)."""
        s_all = -(-T // 32) * 32
        if s_all <= seeded:
            return None
        if precision == torch.float16 or precision == ConditioningStream.SPLIT:
            return None if tail == "mixed" else (seeded, s_all - seeded, min(4, (s_all - seeded) // 32), 1, True)
        mixed_wgs = P * (seeded // 32 + -(-(T - seeded) // 16))
        seeded_wgs = P * (s_all // 32)
        in_kernel = 0 < seeded < T and tail != "seed" and (tail == "mixed" or -(-mixed_wgs // n_cu) <= -(-seeded_wgs // n_cu))
        return None if in_kernel else (seeded, s_all - seeded, 1, 2, False)

    def vocode(self, sigma, z=None, seed=None):
        """WaveGlow.infer of the streamed utterance from the seeds (the frames behind the last block get theirs here, or run
        unseeded: tail_pass); fp32 audio (a half vocoder's is widened as the unstreamed path's is)."""
        n_cu = torch.cuda.get_device_properties(self.dev).multi_processor_count
        s_done = self.seeded
        job = self.tail_pass(self.SPLIT if self.split else self.dtype, self.Tout, s_done, self.waveglow.upsample.stride[0] // 8, n_cu,
                             os.environ.get("FACPPG_STREAM_TAIL"))
        if job is not None:
            frame0, nframes, block_tiles, lpw, bounded = job
            self._seed_pass(frame0, nframes, block_tiles, lpw, n_cu if bounded else None, timed=self.profile)
            s_done = frame0 + nframes
        self.active = False
        audio = self.waveglow.infer_seeded(self._vocoder_mel(), self.Tout, self.seeds, s_done, sigma=sigma, z=z, seed=seed,
                                           handle=self.wg_handle, T_layout=self.cap, flow_events=self.flow_events, **self._kind())
        return audio.float() if self.half else audio


class StageTimer(object):
    """hipEvent timestamps on the launch stream between the stages of one synthesize() call (the kernels run on
    torch's current stream, so torch.cuda.Event brackets them).  ``mark(name)`` closes stage ``name``."""

    def __init__(self):
        self.marks = []
        self.mark("start")

    def mark(self, name):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        self.marks.append((name, ev))

    def stages_ms(self):
        """{stage: ms} in order, plus 'total'; synchronises the last event."""
        self.marks[-1][1].synchronize()
        out = {}
        for (_, a), (name, b) in zip(self.marks[:-1], self.marks[1:]):
            out[name] = out.get(name, 0.0) + a.elapsed_time(b)
        out["total"] = self.marks[0][1].elapsed_time(self.marks[-1][1])
        return out


def pad_ppgs(ppgs, device=None):
    """list of [Tin_i, D] arrays -> ([B, D, Tmax] float32 tensor, lengths list).

    With ``device`` the frames are uploaded as they are (time-major, one contiguous copy each) and
    transposed into the channel-major batch on the GPU; the host-side transpose of a 2 s utterance
    ([200, 5816] floats) costs more than the whole encoder."""
    lens = [int(p.shape[0]) for p in ppgs]
    D = int(ppgs[0].shape[1])
    # (one utterance, or equal lengths: every column is written below -- no zero fill in front of the upload)
    alloc = torch.empty if min(lens) == max(lens) else torch.zeros
    x = alloc(len(ppgs), D, max(lens), dtype=torch.float32, device=device)
    for b, p in enumerate(ppgs):
        t = torch.as_tensor(np.ascontiguousarray(p, dtype=np.float32))
        if device is not None:
            t = t.to(device, non_blocking=True)
        x[b, :, :lens[b]] = t.t()
    return x, lens


def _acoustic(ppgs, tacotron, seed, dropout_masks, utterance_seeds, step_limits, timer=None, while_decoding=None, consumer=None,
              decoder_workgroups=None, consumer_arithmetic=None, prepared=None):
    """PPG upload + Tacotron2.inference on the current stream -> (mel_post [B, 80, Tout], [Tout_i]).  Blocks the host once,
    for the decoder's output lengths.  prepared: (x [B, D, Tmax] on the device, lengths) in place of ``ppgs`` -- the front end's
    own output (ppg.compute_ppg_padded): nothing to upload."""
    dev = next(tacotron.parameters()).device
    if prepared is not None:
        x, lens = prepared
    else:
        x, lens = pad_ppgs(ppgs, device=dev)
        if timer is not None:
            timer.mark("ppg_upload")
    out = tacotron.inference(x, lengths=lens if len(lens) > 1 else None, dropout_masks=dropout_masks,
                             seed=seed, utterance_seeds=utterance_seeds, step_limits=step_limits,
                             while_decoding=while_decoding, frame_consumer=consumer if len(lens) == 1 else None,
                             decoder_workgroups=decoder_workgroups, **({"timer": timer} if timer is not None else {}),
                             **({"frame_consumer_arithmetic": consumer_arithmetic} if consumer_arithmetic is not None and consumer is not None else {}))
    mel_post, tout = out[1], [int(v) for v in out.out_lengths]
    if consumer is not None and consumer.active:      # (the vocoder reads the stream's own mel buffer: no copy on the latency path)
        return mel_post, tout
    return mel_post.contiguous(), tout


def _checked_arithmetic(arithmetic):
    """The ``vocoder_arithmetic`` of a call -> what WaveGlow.infer takes as ``arithmetic`` (None: the module's own path);
    an unknown value is refused here, before any model runs."""
    from waveglow.glow import WaveGlow
    if arithmetic not in WaveGlow.ARITHMETICS:
        from facppg.lib import FacppgError
        raise FacppgError("vocoder_arithmetic=%r: expected None, 'fp32' or 'bf16x3'" % (arithmetic,))
    return None if arithmetic == "fp32" else arithmetic


def _checked_stream(vocoder_stream):
    """The ``vocoder_stream`` of a call: None or True; anything else is refused here, before any model runs."""
    if vocoder_stream is not None and vocoder_stream is not True:
        from facppg.lib import FacppgError
        raise FacppgError("vocoder_stream=%r: expected None or True" % (vocoder_stream,))
    return vocoder_stream


def _vocode(mel_post, tout, waveglow, denoiser, sigma, strength, seed, z, utterance_seeds, timer=None, consumer=None, arithmetic=None,
            split_first=False):
    """WaveGlow.infer + Denoiser on the current stream -> audio [B, Tout_max * hop] on the device; no host waits beyond the
    small uploads (lengths, seeds).  arithmetic: WaveGlow.infer's ("bf16x3": streamed only for the calls that opted in).
    split_first: one utterance of an opt-in "bf16x3" call -- the conditioning-first split path, from the stream's seeds or, when
    the stream did not run, from none (the same samples)."""
    hop = waveglow.upsample.stride[0]
    multi = len(tout) > 1
    wg_seeds = None if utterance_seeds is None else [int(v) + 1 for v in utterance_seeds]
    streamed = consumer is not None and consumer.active
    # a .half() vocoder: half mel in, its half audio widened to fp32 (infer refuses a module that is neither all fp32 nor all fp16)
    half = (consumer.dtype if streamed else ConditioningStream.precision(waveglow, walk=False)) == torch.float16
    if half and not streamed:
        mel_post = mel_post.to(waveglow.upsample.weight.dtype)
    if streamed:
        if wg_seeds is not None:
            z = waveglow.draw_noise(wg_seeds, tout[0], mel_post.device)
        audio = consumer.vocode(sigma, z=z, seed=seed)
    elif split_first:
        if wg_seeds is not None:
            z = waveglow.draw_noise(wg_seeds, tout[0], mel_post.device)
        h = waveglow.handle(mel_post.device, arithmetic)
        melp = waveglow.mel_pad(mel_post[:, :, :tout[0]], handle=h, arithmetic=arithmetic)
        audio = waveglow.infer_seeded(melp, tout[0], None, 0, sigma=sigma, z=z, seed=seed, handle=h, arithmetic=arithmetic)
    else:
        # one utterance through a half vocoder: the K order of the streamed path (conditioning first), so that the samples do not
        # depend on whether this utterance was streamed (too short, FACPPG_STREAM=0, outgrew the layout, stream busy)
        order = {"cond_first": True} if half and not multi else {}
        if arithmetic is not None:
            order["arithmetic"] = arithmetic
        audio = waveglow.infer(mel_post, sigma=sigma, z=z, lengths=tout if multi else None, seed=seed, utterance_seeds=wg_seeds, **order)
        if half:
            audio = audio.float()
    if timer is not None:
        timer.mark("waveglow")
    if denoiser is not None:
        audio = denoiser(audio, strength=strength, lengths=[t * hop for t in tout] if multi else None)[:, 0]
        if timer is not None:
            timer.mark("denoiser")
    return audio


def synthesize(ppgs, tacotron, waveglow, denoiser=None, sigma=0.6, strength=0.005, seed=None, dropout_masks=None, z=None,
               return_device=False, utterance_seeds=None, step_limits=None, timer=None, vocoder_arithmetic=None, vocoder_stream=None):
    """Returns (list of float32 waveforms [N_i], list of mel lengths).  Models must be on the GPU.

    One utterance (the latency path, the metric's "batch = 1"): the postnet and the conditioning part of the vocoder's gate GEMMs
    run while the decoder is still producing frames (ConditioningStream; FACPPG_STREAM=0 switches it off) -- same samples.
    utterance_seeds: one integer per utterance -- its dropout and noise streams then depend on that seed alone,
    so the result for an utterance is the same whatever batch, batch size or GPU it is synthesised in.
    step_limits: per-utterance max_decoder_steps (e.g. its PPG length).
    vocoder_arithmetic: WaveGlow.infer's ``arithmetic`` (None / "fp32": the module's own path; "bf16x3": split-bf16 operands on the
    bf16 MFMA, fp32 samples out).  A plain "bf16x3" call always takes the unstreamed path: ConditioningStream is not used.
    vocoder_stream: None = the above in every respect; True with vocoder_arithmetic="bf16x3" and ONE utterance = the split
    arithmetic in the conditioning-first K order, its conditioning work streamed under the decoder whenever the stream is usable
    (long enough, FACPPG_STREAM not 0, not busy, inside its layout, memory for the seeds) and the same call unseeded when it is
    not: the samples never depend on whether or how far the utterance was streamed; they differ from the plain "bf16x3" call's in
    the last bits (fp32 reassociation, the same accuracy).  True with any other arithmetic changes nothing (those stream by their
    own rules), and a batch of several utterances ignores the keyword and runs as without it -- as a .half() vocoder is
    conditioning-first for one utterance only.  Any other value is refused before a model runs."""
    arithmetic = _checked_arithmetic(vocoder_arithmetic)
    _checked_stream(vocoder_stream)
    if timer is not None:
        timer.__init__()
    return _synthesize(ppgs, None, tacotron, waveglow, denoiser, sigma, strength, seed, dropout_masks, z, return_device, utterance_seeds,
                       step_limits, timer, arithmetic, vocoder_stream)


def _synthesize(ppgs, prepared, tacotron, waveglow, denoiser, sigma, strength, seed, dropout_masks, z, return_device, utterance_seeds,
                step_limits, timer, arithmetic, vocoder_stream):
    """synthesize() behind its argument checks, over host PPGs or over a batch the front end left on the device (``prepared``, see
    _acoustic): the same stages under the same rules either way."""
    n = len(ppgs) if prepared is None else len(prepared[1])
    split_first = vocoder_stream is True and arithmetic == ConditioningStream.SPLIT and n == 1
    hop = waveglow.upsample.stride[0]
    with torch.no_grad():
        dev = next(waveglow.parameters()).device
        consumer = None
        if n == 1 and (arithmetic is None or split_first) and ConditioningStream.usable(tacotron, waveglow):
            consumer = waveglow.__dict__.get("_facppg_cond_stream")
            if consumer is None or consumer.tacotron is not tacotron:
                consumer = waveglow.__dict__["_facppg_cond_stream"] = ConditioningStream(tacotron, waveglow)
        # The stream's buffers and per-utterance state belong to the model pair: ONE utterance at a time goes through them.  A second
        # thread serving another batch-1 request on the same models meanwhile takes the unstreamed path (same samples).
        if consumer is not None and not consumer.lock.acquire(blocking=False):
            consumer = None
        try:
            mel_post, tout = _acoustic(ppgs, tacotron, seed, dropout_masks, utterance_seeds, step_limits, timer,
                                       # host work under the decoder's milliseconds: the vocoder's weight check (the stream does its own)
                                       while_decoding=lambda: None if (consumer is not None and consumer.active) else
                                       (waveglow.prepare(dev, arithmetic) if arithmetic is not None else waveglow.prepare(dev)),
                                       consumer=consumer, consumer_arithmetic=arithmetic if split_first else None, prepared=prepared)
            audio = _vocode(mel_post, tout, waveglow, denoiser, sigma, strength, seed, z, utterance_seeds, timer, consumer, arithmetic,
                            split_first)
        finally:
            if consumer is not None:
                consumer.lock.release()
    if return_device:
        return [audio[b, :tout[b] * hop] for b in range(len(tout))], tout
    host = audio.cpu().numpy()
    return [host[b, :tout[b] * hop].copy() for b in range(len(tout))], tout


def _checked_wav_list(wavs, ppgs, what):
    """``wavs`` is a non-empty list, and no ``ppgs`` came with it."""
    from facppg.lib import FacppgError
    if ppgs is not None:
        raise FacppgError("%s: both ppgs and wavs given -- an utterance comes from one of them" % what)
    if wavs is None or isinstance(wavs, (str, bytes)) or not hasattr(wavs, "__len__") or len(wavs) == 0:
        raise FacppgError("%s: wavs must be a non-empty list of WaveData (common.feat.read_wav_kaldi)" % what)


def _checked_wavs(wavs, deps, tacotron, is_full_ppg, what, ppgs=None):
    """The argument checks of a call that starts from audio, all on the host and before any device work: ``wavs`` a non-empty list
    (and no ``ppgs`` next to it), an acoustic model in ``deps`` whose posteriors -- senone or monophone -- have the width the
    PPG -> mel model was built for, or that width + 3 (a model trained with ``is_append_f0``: _checked_append_f0).  Returns
    is_full_ppg (None: whichever width fits the model's n_symbols)."""
    from facppg.lib import FacppgError
    from ppg.compute_ppg import _require_model, padded_ppg_dim
    _checked_wav_list(wavs, ppgs, what)
    if deps is None:
        raise FacppgError("%s: no PPG dependencies (ppg.DependenciesPPG) -- wavs need the acoustic model" % what)
    _require_model(getattr(deps, "nnet", None), what)
    n_symbols = tacotron._hp["n_symbols"]
    if is_full_ppg is None:
        is_full_ppg = padded_ppg_dim(deps, True) in (n_symbols, n_symbols - 3) or getattr(deps, "monophone_trans", None) is None
    D = padded_ppg_dim(deps, bool(is_full_ppg))
    if n_symbols not in (D, D + 3):
        raise FacppgError("%s: the %s PPGs of these dependencies have %d symbols, the PPG -> mel model was built for %d"
                          % (what, "senone" if is_full_ppg else "monophone", D, n_symbols))
    return bool(is_full_ppg)


def _checked_append_f0(deps, tacotron, is_full_ppg, append_f0, what):
    """Whether the front end appends the three log-F0 rows (ppg.compute_ppg_padded(append_f0=True)): None means on iff the model's
    n_symbols is the PPG width + 3 (hparams.is_append_f0 at training time); a choice the width contradicts is refused.  Host work
    only, after _checked_wavs."""
    from facppg.lib import FacppgError
    from ppg.compute_ppg import padded_ppg_dim
    n_symbols = tacotron._hp["n_symbols"]
    D = padded_ppg_dim(deps, is_full_ppg)
    fits = n_symbols == D + 3
    if append_f0 is None:
        append_f0 = fits
    if bool(append_f0) != fits:
        raise FacppgError("%s: append_f0=%s gives %d input rows (%d %s PPG rows%s), the PPG -> mel model was built for %d"
                          % (what, bool(append_f0), D + (3 if append_f0 else 0), D, "senone" if is_full_ppg else "monophone",
                             " + 3 log-F0 rows" if append_f0 else "", n_symbols))
    return bool(append_f0)


def synthesize_wavs(wavs, deps, tacotron, waveglow, denoiser=None, is_full_ppg=None, sigma=0.6, strength=0.005, seed=None,
                    dropout_masks=None, z=None, return_device=False, utterance_seeds=None, step_limits=None, timer=None,
                    vocoder_arithmetic=None, vocoder_stream=None, ppgs=None, append_f0=None):
    """synthesize() from teacher audio (the reference's purpose, generate_synthesis.py:86-98): wavs, a list of WaveData on the GPU
    (common.feat.read_wav_kaldi), go through the batch front end (ppg.compute_ppg_padded: features, acoustic model of ``deps``,
    a ppg.DependenciesPPG) and their posteriors reach the encoder where the front end left them -- on the device, in the padded
    channel-major batch it reads; no PPG visits the host.  Every keyword of synthesize() means what it means there, the result
    is synthesize()'s, and one utterance takes the streamed batch-1 paths under the same rules.

    is_full_ppg: senone posteriors (True) or monophone PPGs through deps.monophone_trans (False); None picks the one whose width
    is the model's n_symbols.  A width that differs from n_symbols is refused before anything is launched, and so is a call that
    names ``ppgs`` as well: an utterance comes from one of the two.
    append_f0: the front end's F0 track as three more input rows (log F0, delta, delta-delta: ppg.compute_ppg_padded), for a model
    trained with ``is_append_f0``; None: on iff n_symbols is the PPG width + 3.
    The monophone PPGs are compute_ppg_batch's bit for bit, so the samples are those of synthesize() over its host copies; the
    senone posteriors sum their softmax in another order than the row-major output kernels (the same bounds against the
    oracle), so there the samples are those of synthesize() over host copies of compute_ppg_padded's own values."""
    from ppg.compute_ppg import compute_ppg_padded
    is_full_ppg = _checked_wavs(wavs, deps, tacotron, is_full_ppg, "synthesize_wavs", ppgs)
    arithmetic = _checked_arithmetic(vocoder_arithmetic)
    _checked_stream(vocoder_stream)
    append_f0 = _checked_append_f0(deps, tacotron, is_full_ppg, append_f0, "synthesize_wavs")
    if timer is not None:
        timer.__init__()
    with torch.no_grad():
        prepared = compute_ppg_padded(wavs, deps, is_full_ppg=is_full_ppg, append_f0=append_f0)
    if timer is not None:
        timer.mark("front_end")
    return _synthesize(None, prepared, tacotron, waveglow, denoiser, sigma, strength, seed, dropout_masks, z, return_device, utterance_seeds,
                       step_limits, timer, arithmetic, vocoder_stream)


def _preview_seeds(seed, utterance_seeds):
    """The phase seeds of a preview next to its dropout seeds: the decoder draws from ``utterance_seeds[b]`` (or ``seed``), the
    vocoder of synthesize() from utterance_seeds[b] + 1, Griffin-Lim's phases from utterance_seeds[b] + 2 (or seed + 2: STFT.griffin_lim
    then derives one seed per utterance) -- so a corpus keyed by seed + 3 * i never shares a stream between stages."""
    if utterance_seeds is not None:
        return {"utterance_seeds": [int(v) + 2 for v in utterance_seeds]}
    return {"seed": None if seed is None else int(seed) + 2}


def _preview(ppgs, prepared, tacotron, stft, n_iters, momentum, seed, utterance_seeds, step_limits, dropout_masks, return_device):
    if seed is not None and utterance_seeds is not None:
        from facppg.lib import FacppgError
        raise FacppgError("preview: seed and utterance_seeds are two ways to say the same thing -- give one")
    hop = stft.stft_fn.hop_length
    with torch.no_grad():
        mel_post, tout = _acoustic(ppgs, tacotron, seed, dropout_masks, utterance_seeds, step_limits, prepared=prepared)
        audio = stft.griffin_lim(mel_post, lengths=tout, n_iters=n_iters, momentum=momentum, **_preview_seeds(seed, utterance_seeds))[:, 0]
    n = [(t - 1) * hop for t in tout]
    if return_device:
        return [audio[b, :n[b]] for b in range(len(tout))], tout
    host = audio.cpu().numpy()
    return [host[b, :n[b]].copy() for b in range(len(tout))], tout


def preview(ppgs, tacotron, stft, n_iters=60, momentum=0.99, seed=None, utterance_seeds=None, step_limits=None, dropout_masks=None,
            return_device=False, prepared=None):
    """synthesize() without a vocoder: PPGs -> Tacotron2.inference -> TacotronSTFT.griffin_lim (the mel inverted to a linear
    magnitude by the pseudo-inverse of the mel basis, then Griffin-Lim with momentum as one device loop).  Returns (list of float32
    waveforms, list of mel lengths) in synthesize()'s shapes; utterance b has hop * (mel length - 1) samples (the inverse STFT
    of its frames), hop fewer than the vocoder would make.  stft: a common.layers.TacotronSTFT on the model's device, with the
    analysis parameters the model was trained on.
    seed / utterance_seeds: as synthesize() -- the decoder's dropout draws come from them, and the starting phases from the same
    values + 2 (the vocoder's noise of synthesize() takes + 1): with utterance_seeds, utterance b's waveform is that of its own
    batch-1 call.  Giving both is refused.  step_limits, dropout_masks: as synthesize().  prepared: (x [B, D, Tmax] on the device,
    lengths) in place of ``ppgs`` (ppg.compute_ppg_padded's result)."""
    return _preview(ppgs, prepared, tacotron, stft, n_iters, momentum, seed, utterance_seeds, step_limits, dropout_masks, return_device)


def preview_wavs(wavs, deps, tacotron, stft, is_full_ppg=None, n_iters=60, momentum=0.99, seed=None, utterance_seeds=None,
                 step_limits=None, dropout_masks=None, return_device=False, ppgs=None, append_f0=None):
    """preview() from teacher audio, the way synthesize_wavs() starts synthesize(): wavs (list of WaveData) go through the batch
    front end of ``deps`` and their PPGs reach the encoder on the device; is_full_ppg and append_f0 follow synthesize_wavs's rules,
    and the argument errors come before any device work."""
    from ppg.compute_ppg import compute_ppg_padded
    is_full_ppg = _checked_wavs(wavs, deps, tacotron, is_full_ppg, "preview_wavs", ppgs)
    append_f0 = _checked_append_f0(deps, tacotron, is_full_ppg, append_f0, "preview_wavs")
    with torch.no_grad():
        prepared = compute_ppg_padded(wavs, deps, is_full_ppg=is_full_ppg, append_f0=append_f0)
    return _preview(None, prepared, tacotron, stft, n_iters, momentum, seed, utterance_seeds, step_limits, dropout_masks, return_device)


def _checked_job_source(job):
    """A synthesize_stream job's utterances come from ONE of ``ppgs``, ``wavs``, ``prepared``."""
    given = [k for k in ("ppgs", "wavs", "prepared") if job.get(k) is not None]
    if len(given) > 1:
        from facppg.lib import FacppgError
        raise FacppgError("synthesize_stream: both %s given -- a job's utterances come from one of ppgs, wavs, prepared" % " and ".join(given))


_ACOUSTIC_STREAMS = {}


def _acoustic_stream(device):
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _ACOUSTIC_STREAMS:
        _ACOUSTIC_STREAMS[key] = torch.cuda.Stream(device=torch.device("cuda", key))
    return _ACOUSTIC_STREAMS[key]


def synthesize_stream(jobs, tacotron, waveglow, denoiser=None, sigma=0.6, strength=0.005, return_device=True, overlap=True,
                      acoustic_workgroups=32, vocoder_arithmetic=None, ppg_deps=None, is_full_ppg=None, append_f0=None):
    """A sequence of batches, software-pipelined: generator of (waveforms, mel lengths), one per job, in order.

    jobs: iterable of dicts with ``ppgs`` and optionally ``seed``, ``utterance_seeds``, ``step_limits`` (as synthesize()).
    A job may carry ``wavs`` (a list of WaveData, as synthesize_wavs() takes it) in place of ``ppgs``: its front end (features,
    acoustic model of ``ppg_deps``, senone or monophone by ``is_full_ppg`` and with or without the log-F0 rows by ``append_f0``,
    both as in synthesize_wavs()) then runs in front of its
    acoustic model on the same stream, i.e. under the previous batch's vocoder as well, and its PPGs never leave the device.
    The samples of a ``wavs`` job are bit for bit its WaveData, as read_wav_kaldi leaves them: complete before the job is handed over.
    ``wavs`` may also be a callable that returns that list.  It is called when the job's acoustic model is about to be enqueued,
    with the acoustic stream current: a caller that reads its wavs there (read_wav_kaldi uploads from pageable memory, a copy
    the host waits for behind everything queued on the current stream) waits for an idle stream and not for the previous batch's
    vocoder, and holds one batch of audio at a time.  script.synthesize_corpus --device_ppgs reads its batches this way.
    The acoustic model of batch i+1 (PPG upload, encoder, the latency-bound autoregressive decoder, postnet -- a few
    percent of the chip for ~25 ms) runs on its own HIP stream UNDER the vocoder of batch i (MFMA-bound, ~120 ms for 16
    utterances) instead of in front of it.  The host enqueues vocoder i first, then walks through acoustic i+1, whose one
    blocking read (the decoder's output lengths) it would otherwise spend idle.  Every utterance's samples are those of
    synthesize() on the same job: the stages, their inputs and their random streams are the same, only their placement in
    time differs (tests/test_gpu_e2e.py).  overlap=False runs the same jobs back to back on the caller's stream.

    acoustic_workgroups: while overlapped, each acoustic call holds its decoder to this many CUs (unless the model carries a bound
    of its own, Tacotron2.decoder_workgroups).  A decoder workgroup owns its CU's LDS, so the vocoder loses every CU the decoder
    sits on; on the whole chip (240 workgroups for 16 utterances) the two stages merely take turns (146.7 -> 140.2 ms per
    batch), on 32 CUs the decoder takes 60 instead of 18 ms -- still hidden -- and the vocoder keeps 7/8 of the chip
    (128.3 ms; profiles/r03_experiments.txt).  The slice width that goes with the bound cuts the decoder's LSTM sums
    differently: samples then equal those of synthesize() with the same Tacotron2.decoder_workgroups bit for bit, and those
    of the unbounded decoder to rounding.  vocoder_arithmetic: as synthesize().

    A job may also carry ``prepared`` = (x [B, D, Tmax] float32 on the device, lengths) in place of ``ppgs`` or ``wavs``: a padded
    batch that is on the device already (ppg.compute_ppg_padded's result, a batch of synthesize_long's segments).  It goes to the
    acoustic model as a ``wavs`` job's front-end result does.  The acoustic stream does not wait for the caller's: whoever
    produced x on another stream orders the two (synthesize_long does).  A job with more than one of the three keys is refused:
    when the job is drawn, the first one before anything touches the device."""
    arithmetic = _checked_arithmetic(vocoder_arithmetic)
    it = iter(jobs)
    first = next(it, None)
    if first is None:
        return
    _checked_job_source(first)
    dev = next(tacotron.parameters()).device
    hop = waveglow.upsample.stride[0]
    main = torch.cuda.current_stream(dev)
    side = _acoustic_stream(dev) if overlap else main

    def acoustic(job):
        _checked_job_source(job)
        with torch.no_grad(), torch.cuda.stream(side):
            # (the inputs are host arrays, or wavs that are complete: nothing on the caller's stream to wait for -- in particular
            #  not the previous vocoder)
            bound = tacotron.decoder_workgroups or (int(acoustic_workgroups or 0) if overlap else 0)
            prepared = job.get("prepared")
            if prepared is not None:
                prepared[0].record_stream(side)
            wavs = job.get("wavs")
            if wavs is not None:
                from ppg.compute_ppg import compute_ppg_padded
                if callable(wavs):
                    # read here, with the acoustic stream current: read_wav_kaldi's upload comes from pageable memory and waits for
                    # the stream it is queued on -- this one, which is idle, and not the caller's, where the previous vocoder runs
                    wavs = wavs()
                full = _checked_wavs(wavs, ppg_deps, tacotron, is_full_ppg, "synthesize_stream", job.get("ppgs"))
                for w in wavs:
                    if torch.is_tensor(w.data()) and w.data().is_cuda:
                        w.data().record_stream(side)
                with_f0 = _checked_append_f0(ppg_deps, tacotron, full, append_f0, "synthesize_stream")
                prepared = compute_ppg_padded(wavs, ppg_deps, is_full_ppg=full, append_f0=with_f0)
            mel_post, tout = _acoustic(job.get("ppgs"), tacotron, job.get("seed"), None, job.get("utterance_seeds"), job.get("step_limits"),
                                       decoder_workgroups=bound, prepared=prepared)
            done = torch.cuda.Event()
            done.record(side)
        mel_post.record_stream(main)
        return job, mel_post, tout, done

    def finish(audio, tout):
        if return_device:
            return [audio[b, :tout[b] * hop] for b in range(len(tout))], tout
        host = audio.cpu().numpy()
        return [host[b, :tout[b] * hop].copy() for b in range(len(tout))], tout

    ready = acoustic(first)
    previous_vocoder = None
    while ready is not None:
        job, mel_post, tout, done = ready
        main.wait_event(done)
        with torch.no_grad():
            audio = _vocode(mel_post, tout, waveglow, denoiser, sigma, strength, job.get("seed"), None, job.get("utterance_seeds"),
                            arithmetic=arithmetic)
        vocoder_done = torch.cuda.Event()
        vocoder_done.record(main)
        nxt = next(it, None)
        if nxt is not None:
            # The acoustic model (~25-60 ms) is several times faster than the vocoder it hides under: left alone, the host would run
            # the acoustic models of ALL remaining jobs under the first vocoders and queue every vocoder call -- each with its output,
            # noise and workspace buffers -- far ahead of its execution.  One job of look-ahead is all the overlap needs: acoustic
            # i+1 is enqueued when vocoder i-1 has finished, i.e. as vocoder i starts.
            if overlap and previous_vocoder is not None:
                previous_vocoder.synchronize()
            ready = acoustic(nxt)       # enqueued behind nothing on its own stream: runs while the vocoder above does
        else:
            ready = None
        previous_vocoder = vocoder_done
        yield finish(audio, tout)


def _checked_long(tacotron, D, what, pause_rows, max_frames, min_frames, min_pause, pause_threshold, seam_fade, batch_frames, vocoder_arithmetic):
    """The argument checks of a long-form call, all on the host and before any device work -> the call's settings."""
    from facppg import longform
    from facppg.lib import FacppgError
    arithmetic = _checked_arithmetic(vocoder_arithmetic)
    longform.check_plan_args(max_frames, min_frames, min_pause, what)
    fade = int(seam_fade) if isinstance(seam_fade, (int, np.integer)) and not isinstance(seam_fade, bool) else -1
    if fade < 0 or fade > 4096 or fade & (fade - 1):
        raise FacppgError("%s: seam_fade=%r: expected 0 or a power of two up to 4096 (samples; the gains are then exact)" % (what, seam_fade))
    if pause_rows is None:
        if D != 40:
            raise FacppgError("%s: pause_rows is needed for PPGs of %d symbols (only the 40 monophone classes have a known pause row, 39 = sil)"
                              % (what, D))
        pause_rows = [39]
    rows = [int(r) for r in pause_rows]
    if not rows or min(rows) < 0 or max(rows) >= D:
        raise FacppgError("%s: pause_rows must be at least one row in [0, %d) (got %r)" % (what, D, list(pause_rows)))
    if not 0.0 < float(pause_threshold) < float(len(rows)):
        raise FacppgError("%s: pause_threshold=%r is outside (0, %d), the range of a sum of %d posteriors" % (what, pause_threshold, len(rows), len(rows)))
    batch_frames = 16 * int(max_frames) if batch_frames is None else int(batch_frames)
    if batch_frames < 1:
        raise FacppgError("%s: batch_frames must be at least 1 (got %d)" % (what, batch_frames))
    cap = int(tacotron.decoder.max_decoder_steps)
    if int(max_frames) > cap:
        raise FacppgError("%s: max_frames=%d is above the model's max_decoder_steps (%d): such a segment would be cut off" % (what, max_frames, cap))
    return dict(arithmetic=arithmetic, rows=rows, max_frames=int(max_frames), min_frames=int(min_frames), min_pause=int(min_pause),
                threshold=float(pause_threshold), fade=fade, batch_frames=batch_frames)


def pause_flags(x, lengths, rows, threshold):
    """facppg_ppg_pause_flags on the current stream: x [B, D, Tmax] fp32 on the device -> uint8 [B, Tmax] on the device, 1 where
    the frame is inside its recording and its ``rows`` (added in that order in fp32) hold more than ``threshold``."""
    from facppg import lib as _lib
    L = _lib.load()
    _lib.require_cuda(x, "pause_flags: x")
    dev = x.device
    B, D, Tmax = x.shape
    flags = torch.empty(B, Tmax, dtype=torch.uint8, device=dev)
    # (both tables are held until the launch is enqueued: a device tensor that is dropped goes back to the allocator at once, and
    #  the next upload would land in its place)
    lens_dev = _lib.upload([int(n) for n in lengths], torch.int32, dev)
    rows_dev = _lib.upload([int(r) for r in rows], torch.int32, dev)
    with torch.cuda.device(dev):
        _lib.check(L.facppg_ppg_pause_flags(_lib.ptr(x), _lib.ptr(lens_dev), B, D, Tmax, _lib.ptr(rows_dev), _lib.offsets_array(rows), len(rows),
                                            float(threshold), _lib.ptr(flags), _lib.current_stream(dev)))
    return flags


def _synthesize_long(x, lens, cfg, tacotron, waveglow, denoiser, seed, limit_to_input, sigma, strength, return_device, overlap,
                     acoustic_workgroups):
    """synthesize_long() behind its argument checks, over the padded device batch (x [B, D, Tmax], lens)."""
    from facppg import lib as _lib
    from facppg import longform
    L = _lib.load()
    _lib.require_cuda(x, "synthesize_long: the PPG batch")
    dev = x.device
    x = x.float().contiguous()
    B, D, Tmax = x.shape
    hop = waveglow.upsample.stride[0]
    with torch.no_grad(), torch.cuda.device(dev):
        st = _lib.current_stream(dev)
        flags = pause_flags(x, lens, cfg["rows"], cfg["threshold"]).cpu().numpy()      # one byte per frame: the call's only added host wait
        plans = [longform.plan_segments(flags[b, :lens[b]], cfg["max_frames"], cfg["min_frames"], cfg["min_pause"]) for b in range(B)]
        pooled = [(b, s, n) for b, plan in enumerate(plans) for s, n in plan]
        jobs = []
        for i, j in longform.group_segments([p[2] for p in pooled], cfg["batch_frames"]):
            flat = [v for p in pooled[i:j] for v in p]
            frames = [p[2] for p in pooled[i:j]]
            y = torch.empty(j - i, D, max(frames), dtype=torch.float32, device=dev)
            table = _lib.upload(flat, torch.int32, dev)
            _lib.check(L.facppg_ppg_gather_segments(_lib.ptr(x), B, D, Tmax, _lib.ptr(table), _lib.offsets_array(flat), j - i, max(frames),
                                                    _lib.ptr(y), st))
            job = dict(prepared=(y, frames), utterance_seeds=[seed + 2 * k for k in range(i, j)])
            if limit_to_input:
                job["step_limits"] = frames
            jobs.append(job)
        if overlap:           # the acoustic models run on a stream of their own, which has to see the gathers above
            _acoustic_stream(dev).wait_stream(torch.cuda.current_stream(dev))
        audio, tout = [], []
        for a, t in synthesize_stream(jobs, tacotron, waveglow, denoiser, sigma=sigma, strength=strength, return_device=True, overlap=overlap,
                                      acoustic_workgroups=acoustic_workgroups, vocoder_arithmetic=cfg["arithmetic"]):
            audio += a
            tout += t
        waveforms, tables, k = [], [], 0
        for plan in plans:
            S = len(plan)
            n = [tout[k + s] * hop for s in range(S)]
            stacked = torch.nn.utils.rnn.pad_sequence(audio[k:k + S], batch_first=True).contiguous()
            out = torch.empty(sum(n), dtype=torch.float32, device=dev)
            n_dev = _lib.upload(n, torch.int32, dev)
            _lib.check(L.facppg_join_segments(_lib.ptr(stacked), stacked.shape[1], _lib.ptr(n_dev), _lib.offsets_array(n), S, cfg["fade"],
                                              _lib.ptr(out), st))
            waveforms.append(out)
            tables.append([(s0, fr, tout[k + s]) for s, (s0, fr) in enumerate(plan)])
            k += S
    if not return_device:
        waveforms = [w.cpu().numpy() for w in waveforms]
    return waveforms, tables


def synthesize_long(ppgs, tacotron, waveglow, denoiser=None, *, pause_rows=None, max_frames=600, min_frames=150, min_pause=8,
                    pause_threshold=0.5, seam_fade=64, batch_frames=None, seed=0, limit_to_input=False, sigma=0.6, strength=0.005,
                    return_device=False, vocoder_arithmetic=None, overlap=True, acoustic_workgroups=32):
    """Recordings of any length -> (waveforms, segment tables).  Tacotron2.inference decodes at most max_decoder_steps frames
    (about ten seconds) and cuts a longer recording off, as the reference does (model.py:527); here a recording is cut at its
    pauses where the posteriors already lie, the pieces are converted as padded batches under synthesize_stream, and their audio
    is joined on the device.  One byte per frame visits the host.

    ppgs: a list of recordings, host [T, D] arrays, or ONE device batch (x [B, D, Tmax], lengths) as ppg.compute_ppg_padded
    leaves it.  The PPG of the whole recording is computed before it is cut, so the acoustic model's context crosses the cuts.
    pause_rows: the PPG rows that mean "pause"; their fp32 sum, in this order, above ``pause_threshold`` flags a frame
    (facppg_ppg_pause_flags).  None: [39], the monophone PPG's ``sil``, when D == 40; refused otherwise.
    max_frames / min_frames / min_pause: facppg.longform.plan_segments' (no segment longer than max_frames, none shorter than
    min_frames once there are several, pauses of at least min_pause frames).  max_frames above the model's max_decoder_steps is
    refused.  The defaults are policy (6 s segments, 80 ms pauses, 4 ms fades), not measurements.
    batch_frames: the pooled segments -- (recording, segment) order -- are grouped greedily, a group the longest run of
    consecutive segments with count * longest <= batch_frames (None: 16 * max_frames) and at least one; each group is gathered
    into a fresh [S, D, Lmax] batch (facppg_ppg_gather_segments) and runs as one ``prepared`` job of synthesize_stream
    (``overlap`` / ``acoustic_workgroups`` / ``vocoder_arithmetic`` are its keywords).
    seed: segment j in pooled order gets utterance seed ``seed + 2 * j``; the vocoder draws its noise from that seed + 1, so the
    stride keeps the streams apart.  limit_to_input: each segment's frame count is its step limit (the reference's is_clip idea);
    otherwise the gate ends it.
    seam_fade: samples of linear fade on either side of every interior seam (facppg_join_segments: 0 or a power of two up to
    4096, shortened for short segments); lengths are additive, nothing overlaps.
    The table of a recording lists (start, frames, mel_length) per segment; its waveform has hop * sum(mel_length) samples.
    Every argument check runs on the host before anything touches a device."""
    from facppg.lib import FacppgError
    what = "synthesize_long"
    batch = isinstance(ppgs, tuple) and len(ppgs) == 2 and torch.is_tensor(ppgs[0])
    if batch:
        x, lens = ppgs[0], [int(n) for n in ppgs[1]]
        if x.dim() != 3 or len(lens) != x.shape[0] or not lens or min(lens) < 1 or max(lens) > x.shape[2]:
            raise FacppgError("%s: a device batch is (x [B, D, Tmax], B lengths in [1, Tmax])" % what)
        D = int(x.shape[1])
    else:
        if ppgs is None or not hasattr(ppgs, "__len__") or len(ppgs) == 0:
            raise FacppgError("%s: ppgs must be a non-empty list of [T, D] arrays, or one device batch (x, lengths)" % what)
        D = int(ppgs[0].shape[1])
    cfg = _checked_long(tacotron, D, what, pause_rows, max_frames, min_frames, min_pause, pause_threshold, seam_fade, batch_frames,
                        vocoder_arithmetic)
    if not batch:
        x, lens = pad_ppgs(ppgs, device=next(tacotron.parameters()).device)
    return _synthesize_long(x, lens, cfg, tacotron, waveglow, denoiser, int(seed), limit_to_input, sigma, strength, return_device, overlap,
                            acoustic_workgroups)


def synthesize_long_wavs(wavs, deps, tacotron, waveglow, denoiser=None, is_full_ppg=None, *, pause_rows=None, max_frames=600, min_frames=150,
                         min_pause=8, pause_threshold=0.5, seam_fade=64, batch_frames=None, seed=0, limit_to_input=False, sigma=0.6,
                         strength=0.005, return_device=False, vocoder_arithmetic=None, overlap=True, acoustic_workgroups=32, append_f0=None):
    """synthesize_long() from teacher audio: wavs (a list of WaveData, whole recordings) go through ppg.compute_ppg_padded once and
    its device batch is cut, converted and joined as above; no posterior visits the host.  is_full_ppg and append_f0 as in
    synthesize_wavs(): with the log-F0 rows the segments carry K + 3 rows, and their delta rows are those of the WHOLE recording (a
    segment's first frame keeps the slope it had there).
    pause_rows None: [39] for monophone PPGs; for senone PPGs the senones that ``deps.monophone_trans`` maps to row 39 (its
    nonzero columns: the same mass), refused when the dependencies have no such map."""
    from facppg.lib import FacppgError
    from ppg.compute_ppg import compute_ppg_padded
    what = "synthesize_long_wavs"
    is_full_ppg = _checked_wavs(wavs, deps, tacotron, is_full_ppg, what)
    if pause_rows is None:
        if not is_full_ppg:
            pause_rows = [39]
        else:
            trans = getattr(deps, "monophone_trans", None)
            if trans is None or trans.shape[0] <= 39:
                raise FacppgError("%s: pause_rows is needed for senone PPGs when the dependencies have no pdf -> monophone matrix "
                                  "(data/feats/reduce_dim.mat) to read the pause senones from" % what)
            pause_rows = [int(c) for c in torch.nonzero(torch.as_tensor(trans)[39]).flatten()]
    cfg = _checked_long(tacotron, tacotron._hp["n_symbols"], what, pause_rows, max_frames, min_frames, min_pause, pause_threshold, seam_fade,
                        batch_frames, vocoder_arithmetic)
    append_f0 = _checked_append_f0(deps, tacotron, is_full_ppg, append_f0, what)
    with torch.no_grad():
        x, lens = compute_ppg_padded(wavs, deps, is_full_ppg=is_full_ppg, append_f0=append_f0)
    return _synthesize_long(x, lens, cfg, tacotron, waveglow, denoiser, int(seed), limit_to_input, sigma, strength, return_device, overlap,
                            acoustic_workgroups)
