"""MI355X-native SMILES-VAE training hot path (drop-in for aclyde11/molecular-VAE's models.py / train.py surface).

The directory name (``molecular-vae_amd``) is fixed by the repo layout contract and is not a Python identifier;
import it through the ``molecular_vae_amd`` alias package at the repo root.
"""
from . import _lib  # noqa: F401
from .models import (MolecularVAE, MolEncoder, MolDecoder, Lambda, ConvSELU, SELU, TimeDistributed, Repeat,  # noqa: F401
                     Flatten)
from .functional import bce_kl_loss, make_loss_function, decoder_elbo  # noqa: F401
from . import mosesvae, models2d, vocab, data  # noqa: F401
from .data import MoleLoader, DeviceDataset, MosesDeviceDataset, MosesLatentIndex, tokenize_corpus, moses_epoch_plan, build_vocab, encode_smiles, synthetic_smiles, indices_to_smiles, randomized_smiles, canonical_smiles, normal_smiles, selfies_from_smiles, smiles_from_selfies, scaffold_smiles, fragment_smiles, compile_substructures, SubstructureTable  # noqa: F401
from .vocab import CharVocab, OneHotVocab, SelfiesVocab, PaddedBatch, pad_batch, get_collate_fn, get_padded_collate_fn  # noqa: F401
from .train import (FusedAdam, FusedSGD, GradSync, ShardedSampler, shard_batch, train_step, elbo_train_step, exact_match_accuracy,  # noqa: F401
                    evaluate, evaluate_elbo, save_checkpoint, load_checkpoint, strip_module_prefix, KLAnnealer, CyclicalKLAnnealer, CosineAnnealingLRWithRestart, cosine_lr_with_restart,
                    moses_train_step, moses_train_epoch, moses_reconstruction, moses_generate, moses_latent_diagnostics, generate_from_latent)

__all__ = ["mosesvae", "models2d", "vocab", "data", "MoleLoader", "DeviceDataset", "MosesDeviceDataset", "MosesLatentIndex", "tokenize_corpus", "moses_epoch_plan", "build_vocab", "encode_smiles", "CharVocab", "OneHotVocab", "MolecularVAE", "MolEncoder", "MolDecoder", "Lambda", "ConvSELU", "SELU", "TimeDistributed", "Repeat",
           "Flatten", "bce_kl_loss", "make_loss_function", "decoder_elbo", "FusedAdam", "FusedSGD", "GradSync", "ShardedSampler", "shard_batch",
           "train_step", "elbo_train_step", "exact_match_accuracy", "evaluate", "evaluate_elbo", "save_checkpoint", "load_checkpoint", "strip_module_prefix", "KLAnnealer", "CyclicalKLAnnealer",
           "CosineAnnealingLRWithRestart", "cosine_lr_with_restart", "moses_train_step", "moses_train_epoch", "moses_reconstruction", "moses_generate", "moses_latent_diagnostics", "generate_from_latent", "synthetic_smiles", "indices_to_smiles"]
