"""The reference's ``ppg`` package (src/ppg): see compute_ppg.py for what is built, compute_f0.py for the F0 track."""
from ppg.compute_f0 import F0Options, compute_f0, compute_f0_batch, compute_nccf_batch  # noqa: F401
from ppg.compute_ppg import (DependenciesPPG, compute_feat_for_nnet, compute_feat_for_nnet_internal, compute_full_ppg,  # noqa: F401
                             compute_full_ppg_wrapper, compute_monophone_ppg, reduce_ppg_dim, compute_feat_for_nnet_batch,
                             compute_full_ppg_batch, compute_ppg_batch, compute_ppg_padded)
