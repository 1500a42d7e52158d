"""GPU: the denoiser's framing kernel on utterances shorter than half the STFT filter (fl / 2 = 512 samples): the reflected index
2 (Nb - 1) - j leaves such an utterance at its other end, so it is held inside the utterance.  A ragged batch that contains
such utterances (one frame of 10 ms audio, as the wav -> wav tests synthesise) gives each the samples it has with no neighbour
in the batch, whatever the buffer holds behind it, and leaves its long neighbours alone."""
import numpy as np
import pytest
import torch

from facppg import synth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("hop", [160, 256])
def test_denoiser_ragged_batch_with_utterances_shorter_than_half_the_filter(hop):
    from waveglow.denoiser import Denoiser
    from waveglow.glow import WaveGlow
    cfg = dict(synth.WAVEGLOW_CONFIG, hop_length=hop)
    m = WaveGlow.remove_weightnorm(WaveGlow(**cfg))
    m.load_state_dict(synth.waveglow_state_dict(cfg))
    den = Denoiser(m.cuda().eval(), filter_length=1024, hop_length=hop, win_length=1024, mode="zeros")
    g = np.random.Generator(np.random.PCG64(5))
    # one frame first (the reflection would reach in front of the buffer), then 2, 3 and 4 frames behind a long utterance (into
    # the neighbour): at hop 160 the first three need the hold (<= 512 samples), at hop 256 the first two (512 is the last length
    # that does); the others are the first lengths that do not
    N = 25 * hop
    lens = [hop, N, 2 * hop, 3 * hop, 4 * hop]
    x = torch.from_numpy(g.standard_normal((len(lens), N), dtype=np.float32) * 0.2).cuda()
    out = den(x, strength=0.1, lengths=lens)
    assert bool(torch.isfinite(out).all())
    for b, n in enumerate(lens):
        alone = den(x[b:b + 1].contiguous(), strength=0.1, lengths=[n])      # the utterance with no neighbour
        assert alone.shape == (1, 1, N) and bool(torch.isfinite(alone).all())
        assert torch.equal(alone[0, 0], out[b, 0]), (b, n)
        assert bool(out[b, 0, :n].any()) and not bool(out[b, 0, n:].any()), (b, n)
    # the held index reads the utterance's own samples: whatever lies behind them does not matter
    y = x.clone()
    for b, n in enumerate(lens):
        y[b, n:] = 1e4
    assert torch.equal(den(y, strength=0.1, lengths=lens), out)
