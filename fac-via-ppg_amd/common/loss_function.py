"""``Tacotron2Loss`` -- drop-in for src/common/loss_function.py:36-53.

Two MSE means over the padded mel tensors (decoder output and postnet output against the target) plus
BCE-with-logits on the gate energies, weighted ``mel_weight`` and ``gate_weight``.  Not a hot path: plain torch
ops on whatever device the tensors are on, so it scores ``Tacotron2.forward``'s GPU outputs and CPU tensors alike.
"""
from torch import nn


class Tacotron2Loss(nn.Module):
    def __init__(self, mel_weight=1, gate_weight=0.005):
        super(Tacotron2Loss, self).__init__()
        self.w_mel = mel_weight
        self.w_gate = gate_weight

    def forward(self, model_output, targets):
        mel_target, gate_target = targets[0].detach(), targets[1].detach()
        mel_out, mel_out_postnet, gate_out, _ = model_output
        mel_loss = nn.functional.mse_loss(mel_out, mel_target) + nn.functional.mse_loss(mel_out_postnet, mel_target)
        gate_loss = nn.functional.binary_cross_entropy_with_logits(gate_out.reshape(-1, 1), gate_target.reshape(-1, 1))
        return self.w_mel * mel_loss + self.w_gate * gate_loss
