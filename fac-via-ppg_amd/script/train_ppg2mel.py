"""The reference's src/script/train_ppg2mel.py on the HIP kernels: ``load_model`` (:113-119, imported by
generate_synthesis.py:20), ``warm_start_model`` (:122-127), ``load_checkpoint`` / ``save_checkpoint`` (:130-150),
``validate`` (:152-177), which scores a checkpoint on held-out data through the teacher-forced ``Tacotron2.forward`` and
``Tacotron2Loss``, ``validate_free_running``, which scores it the way it converts -- the free-running decoder's mels against the
targets by a mel-cepstral DTW, and what its attention did (no counterpart in the reference) --, and ``finetune``: the body of
the training loop (:199-276) for one GPU with EVAL-MODE semantics, on the backward pass of
``Tacotron2.forward(..., differentiable=True)``.  ``train`` itself is not built: training-mode BatchNorm and the training-mode
dropouts have no kernels."""
import math
import os
import time

import torch
from torch.utils.data import DataLoader
from torch.utils.data.distributed import DistributedSampler

from common.model import Tacotron2


def load_model(hparams):
    if hparams.fp16_run:
        raise NotImplementedError("fp16_run is not built (README.md:53 of the reference: FP16 does not work)")
    return Tacotron2(hparams).cuda()


def warm_start_model(checkpoint_path, model):
    """Initialise ``model`` from the ``'state_dict'`` entry of a training checkpoint (the reference's
    train_ppg2mel.py:122-127); the optimiser state and iteration count in the file are ignored.  Returns the model."""
    if not os.path.isfile(checkpoint_path):
        raise FileNotFoundError("warm_start_model: no checkpoint at %r" % (checkpoint_path,))
    print("Warm starting model from checkpoint '{}'".format(checkpoint_path))
    weights = torch.load(checkpoint_path, map_location="cpu", weights_only=False)["state_dict"]
    model.load_state_dict(weights)                     # (drops the packed-weight handle: Tacotron2.load_state_dict)
    return model


def load_checkpoint(checkpoint_path, model, optimizer):
    """train_ppg2mel.py:130-140: -> (model, optimizer, learning_rate, iteration) from a file of ``save_checkpoint``."""
    if not os.path.isfile(checkpoint_path):
        raise FileNotFoundError("load_checkpoint: no checkpoint at %r" % (checkpoint_path,))
    print("Loading checkpoint '{}'".format(checkpoint_path))
    checkpoint_dict = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
    model.load_state_dict(checkpoint_dict["state_dict"])          # (drops the packed-weight handle)
    optimizer.load_state_dict(checkpoint_dict["optimizer"])
    learning_rate, iteration = checkpoint_dict["learning_rate"], checkpoint_dict["iteration"]
    print("Loaded checkpoint '{}' from iteration {}".format(checkpoint_path, iteration))
    return model, optimizer, learning_rate, iteration


def save_checkpoint(model, optimizer, learning_rate, iteration, filepath):
    """train_ppg2mel.py:143-149, the reference's file layout: iteration, state_dict, optimizer, learning_rate."""
    print("Saving model and optimizer state at iteration {} to {}".format(iteration, filepath))
    torch.save({"iteration": iteration, "state_dict": model.state_dict(), "optimizer": optimizer.state_dict(),
                "learning_rate": learning_rate}, filepath)


def finetune(model, hparams, trainset, collate_fn, steps, output_directory=None, valset=None, checkpoint_path=None,
             warm_start=False, step_seeds=None, step_masks=None, optimizer=None, logger=None, log=print, free_running=False):
    """Fit ``model`` to ``trainset`` for ``steps`` optimiser steps: the body of the reference's training loop
    (train_ppg2mel.py:199-276) on one GPU -- Adam (``waveglow.optim.Adam``, one HIP launch per step) with
    ``hparams.learning_rate`` / ``weight_decay``, zero_grad -> parse_batch -> forward -> Tacotron2Loss -> backward ->
    clip_grad_norm_(``hparams.grad_clip_thresh``) -> step, and ``validate`` + a checkpoint ``checkpoint_<iteration>`` in
    ``output_directory`` every ``hparams.iters_per_checkpoint`` iterations (when an output directory is given; ``validate``
    when a ``valset`` is given).

    THE MODEL STAYS IN EVAL MODE.  The gradient is that of the function ``Tacotron2.forward`` computes in eval mode, the one
    ``validate`` reports the loss of: BatchNorm normalises with its RUNNING statistics, which are not updated (frozen
    normalisation statistics; the BatchNorm weights and biases are trained), and the reference's training-mode dropouts -- 0.5
    behind the encoder convolutions and the postnet layers, 0.1 on the LSTMCell states -- are OFF; the prenets' always-on
    dropouts are on, as everywhere.  The reason is that training-mode semantics have no kernels: ``train()`` stays unbuilt.

    trainset     any map-style data set of (ppg [L_in, n_symbols], acoustic [L_out, n_feat]) pairs; batches of
                 ``hparams.batch_size`` are taken IN ORDER (no shuffling: a run is reproducible) through ``collate_fn``
                 (``common.data_utils.ppg_acoustics_collate``), epoch after epoch
    step_seeds   None, or a callable step -> seed of that step's dropout draws (``Tacotron2.forward(seed=...)``)
    step_masks   None, or a callable step -> (enc masks, dec masks) as ``Tacotron2.forward(dropout_masks=...)`` takes them
    checkpoint_path / warm_start   initialise from a checkpoint's weights (warm start) or resume it: weights, optimiser state,
                 iteration (and its learning rate when ``hparams.use_saved_learning_rate``)
    optimizer    None (built here) or the optimiser to use and resume into
    free_running True: next to ``validate``, every checkpoint is also scored the way it converts (``validate_free_running`` on
                 ``valset``, which it therefore needs); the training steps do not depend on it
    Returns a dict: losses and grad_norms (pre-clip) per step, iteration (the next one), optimizer, learning_rate, and
    free_running: a list of (iteration, validate_free_running's result), empty without the flag."""
    from common.loss_function import Tacotron2Loss
    from waveglow.optim import Adam
    if hparams.fp16_run:
        raise NotImplementedError("finetune: fp16_run is not built (README.md:53 of the reference: FP16 does not work)")
    if free_running and valset is None:
        raise ValueError("finetune: free_running=True scores the checkpoints on a valset, and none was given")
    if any(not p.is_cuda for p in model.parameters()):
        raise ValueError("finetune: the model must be on the GPU (there is no CPU path): load_model(hparams)")
    if step_seeds is not None and step_masks is not None:
        raise ValueError("finetune: step_seeds or step_masks, not both")
    learning_rate = hparams.learning_rate
    if optimizer is None:
        optimizer = Adam(model.parameters(), lr=learning_rate, weight_decay=hparams.weight_decay)
    criterion = Tacotron2Loss(hparams.mel_weight, hparams.gate_weight)
    iteration = 0
    if checkpoint_path:
        if warm_start:
            model = warm_start_model(checkpoint_path, model)
        else:
            model, optimizer, saved_lr, iteration = load_checkpoint(checkpoint_path, model, optimizer)
            if hparams.use_saved_learning_rate:
                learning_rate = saved_lr
            iteration += 1                                        # next iteration is iteration + 1
    if output_directory:
        os.makedirs(output_directory, exist_ok=True)
    batches = DataLoader(trainset, batch_size=hparams.batch_size, shuffle=False, collate_fn=collate_fn, num_workers=0)
    if len(batches) == 0:
        raise ValueError("finetune: the training set yields no batch")
    model.eval()
    losses, norms, free_runs, done = [], [], [], 0
    while done < steps:
        for batch in batches:
            if done == steps:
                break
            start = time.perf_counter()
            for group in optimizer.param_groups:
                group["lr"] = learning_rate
            model.zero_grad()
            x, y = model.parse_batch(batch)
            kw = {}
            if step_seeds is not None:
                kw["seed"] = int(step_seeds(done))
            if step_masks is not None:
                kw["dropout_masks"] = step_masks(done)
            loss = criterion(model(x, differentiable=True, **kw), y)
            reduced_loss = loss.item()
            loss.backward()
            grad_norm = float(torch.nn.utils.clip_grad_norm_(model.parameters(), hparams.grad_clip_thresh))
            optimizer.step()
            # waveglow.optim.Adam's launch writes the parameters through raw pointers: no tensor version moves, so the packed-weight
            # handle (facppg.lib.WeightIdentity) cannot see the step.  Drop it; the next forward packs the new weights.
            model.invalidate_packed_weights()
            losses.append(reduced_loss)
            norms.append(grad_norm)
            if not math.isnan(reduced_loss) and log is not None:
                duration = time.perf_counter() - start
                log("Train loss {} {:.6f} Grad Norm {:.6f} {:.2f}s/it".format(iteration, reduced_loss, grad_norm, duration))
                if logger is not None:
                    logger.log_training(reduced_loss, grad_norm, learning_rate, duration, iteration)
            if output_directory and iteration % hparams.iters_per_checkpoint == 0:
                if valset is not None:
                    validate(model, criterion, valset, iteration, hparams.batch_size, 1, collate_fn, logger, False, 0)
                    model.eval()                                  # (validate leaves train() mode, as the reference does)
                    if free_running:
                        free_runs.append((iteration, validate_free_running(model, valset, hparams.batch_size, logger=logger,
                                                                           iteration=iteration)))
                save_checkpoint(model, optimizer, learning_rate, iteration, os.path.join(output_directory, "checkpoint_{}".format(iteration)))
            iteration += 1
            done += 1
    return {"losses": losses, "grad_norms": norms, "iteration": iteration, "optimizer": optimizer, "learning_rate": learning_rate,
            "free_running": free_runs}


def validate(model, criterion, valset, iteration, batch_size, n_gpus, collate_fn, logger, distributed_run, rank):
    """Score ``model`` on ``valset`` with ``criterion`` through the teacher-forced ``Tacotron2.forward`` -- the reference's
    train_ppg2mel.py:152-177, same signature and print-out.  The result, which is also returned, is the mean over the
    batches of the per-batch loss (averaged over the ranks when ``distributed_run``).  The model is in eval mode during the
    pass and in train() mode afterwards, as the reference leaves it; ``logger`` may be None.
    The batches are taken in the data set's order.  The reference shuffles them, which deals the utterances into other
    padded batches from call to call; with the padded-batch semantics of ``forward`` that moves the loss, so a repeatable
    score needs a fixed order."""
    sampler = DistributedSampler(valset, shuffle=False) if distributed_run else None
    batches = DataLoader(valset, batch_size=batch_size, sampler=sampler, shuffle=False, collate_fn=collate_fn, num_workers=0)
    losses = []
    targets = outputs = None
    model.eval()
    try:
        with torch.no_grad():
            for batch in batches:
                inputs, targets = model.parse_batch(batch)
                outputs = model(inputs)
                batch_loss = criterion(outputs, targets)
                if distributed_run:
                    from waveglow.distributed import reduce_tensor
                    batch_loss = reduce_tensor(batch_loss.detach(), n_gpus)
                losses.append(float(batch_loss))
    finally:
        model.train()
    if not losses:
        raise ValueError("validate: the validation set yields no batch")
    mean_loss = sum(losses) / len(losses)
    if rank == 0:
        print("Validation loss {}: {:9f}  ".format(iteration, mean_loss))
        if logger is not None:
            logger.log_validation(mean_loss, model, targets, outputs, iteration)
    return mean_loss


FREE_RUNNING_FIELDS = ("mcd", "stretch", "frames", "target_frames", "stopped", "first", "last", "back", "max_jump", "longest_stall",
                       "visited", "focus", "coverage", "end_gap")


def validate_free_running(model, valset, batch_size, seed=0, n_cep=13, band=0, step_factor=None, logger=None, iteration=0, rank=0):
    """Score ``model`` on ``valset`` the way it converts: the decoder runs FREE (``Tacotron2.inference``, prenet dropouts on), where it
    can skip, repeat or babble up to its step limit -- none of which the teacher-forced loss of ``validate`` sees.  No counterpart
    in the reference.

    valset[k] = (ppg [L_in, n_symbols], acoustic [L_out, n_feat]) is taken IN ORDER in batches of ``batch_size``, padded here (the
    collate function sorts by length and so loses k).  Utterance k is decoded with ``utterance_seeds = seed + k``: its result does
    not depend on the batch size.  Its step limit is ``max_decoder_steps``, with ``step_factor`` min(that, ceil(step_factor *
    L_out)).  ``mel_post`` is scored against the target mel by ``facppg.score.mel_dtw`` (n_cep, band: this build's own
    mel-cepstral DTW, values compare within this build only) and the alignments by ``facppg.score.attention_path``.
    Returns a dict: per utterance, in valset order, the arrays mcd, stretch, frames, target_frames, stopped (frames < limit: the
    gate ended the utterance, not the limit) and attention_path's first, last, back, max_jump, longest_stall, visited, focus,
    coverage, end_gap; and the aggregates mean_mcd, stopped_share, mean_coverage.
    The model is in eval mode during the pass and is put back into the mode it was found in.  Rank 0 prints one line."""
    import numpy as np
    from facppg import score
    if int(batch_size) < 1:
        raise ValueError("validate_free_running: batch_size must be at least 1 (got %r)" % (batch_size,))
    if step_factor is not None and not float(step_factor) > 0.0:
        raise ValueError("validate_free_running: step_factor must be positive (got %r)" % (step_factor,))
    n = len(valset)
    if n == 0:
        raise ValueError("validate_free_running: the validation set is empty")
    dev = next(model.parameters()).device
    max_steps = int(model.decoder.max_decoder_steps)
    rows = {name: [] for name in FREE_RUNNING_FIELDS}
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for at in range(0, n, int(batch_size)):
                items = [valset[k] for k in range(at, min(at + int(batch_size), n))]
                B = len(items)
                ppgs, mels = [torch.as_tensor(p).float() for p, _ in items], [torch.as_tensor(m).float() for _, m in items]
                tin, ttgt = [int(p.shape[0]) for p in ppgs], [int(m.shape[0]) for m in mels]
                x = torch.zeros(B, ppgs[0].shape[1], max(tin))
                y = torch.zeros(B, mels[0].shape[1], max(ttgt))
                for b in range(B):
                    x[b, :, :tin[b]] = ppgs[b].t()
                    y[b, :, :ttgt[b]] = mels[b].t()
                limits = [max_steps if step_factor is None else max(1, min(max_steps, int(math.ceil(float(step_factor) * t)))) for t in ttgt]
                out = model.inference(x.to(dev), lengths=tin, utterance_seeds=[int(seed) + k for k in range(at, at + B)], step_limits=limits)
                frames = [int(v) for v in out.out_lengths]
                dtw = score.mel_dtw(out[1], frames, y.to(dev), ttgt, n_cep=n_cep, band=band)
                path = score.attention_path(out[3], frames, tin)
                rows["mcd"].append(dtw["mcd"])
                rows["stretch"].append(dtw["stretch"])
                rows["frames"].append(np.asarray(frames, dtype=np.int32))
                rows["target_frames"].append(np.asarray(ttgt, dtype=np.int32))
                rows["stopped"].append(np.asarray(frames) < np.asarray(limits))
                for name in FREE_RUNNING_FIELDS[5:]:
                    rows[name].append(path[name])
    finally:
        model.train(was_training)
    result = {name: np.concatenate(parts) for name, parts in rows.items()}
    result["mean_mcd"] = float(result["mcd"].mean())
    result["stopped_share"] = float(result["stopped"].mean())
    result["mean_coverage"] = float(result["coverage"].mean())
    if rank == 0:
        print("Free-running {}: MCD {:.4f} dB, stopped {:.3f}, coverage {:.3f}".format(iteration, result["mean_mcd"], result["stopped_share"],
                                                                                     result["mean_coverage"]))
        if logger is not None and hasattr(logger, "log_free_running"):
            logger.log_free_running(result, iteration)
    return result


def train(*args, **kwargs):
    raise NotImplementedError("train() is not built: training-mode semantics (batch-statistics BatchNorm, the training-mode "
                              "dropouts) have no kernels.  finetune() fits a checkpoint with eval-mode semantics; validate() "
                              "scores one through the teacher-forced forward pass")
