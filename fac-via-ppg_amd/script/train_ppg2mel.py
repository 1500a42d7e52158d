"""The parts of the reference's src/script/train_ppg2mel.py that need no backward pass: ``load_model`` (:113-119,
imported by generate_synthesis.py:20), ``warm_start_model`` (:122-127) and ``validate`` (:152-177), which scores a
checkpoint on held-out data through the teacher-forced ``Tacotron2.forward`` and ``Tacotron2Loss``.  ``train`` itself is
not built: the kernels have no backward pass."""
import os

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


def train(*args, **kwargs):
    raise NotImplementedError("training the PPG->mel model is not built: the HIP kernels have no backward pass.  "
                              "validate() scores a checkpoint through the teacher-forced forward pass")
