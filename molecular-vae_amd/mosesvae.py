"""Host-side mirror of ``mosesvae.VAE`` (mosesvae.py:27-199): GRU encoder / 3-layer GRU decoder character VAE.

Same constructor (``VAE(vocab)``), hard-coded hyper-parameters (mosesvae.py:31-40), attribute names, aliasing ``ModuleList``s
(88 ``state_dict`` keys over 29 tensors) and ``forward`` 6-tuple ``(kl_loss, recon_loss, z, logvar, x, y)`` as the reference.
The whole forward is one ``torch.autograd.Function`` over the C ABI: embedding folded into the layer-0 GRU input projection
(a table gather), wavefront GRU kernels with per-sequence length masking (== pack_sequence / pad_packed_sequence semantics:
a finished sequence keeps its state and emits zeros), fused heads + reparameterisation + KL, fused token cross-entropy.

Train mode (``model.train()``): the decoder GRU's inter-layer dropout (``d_dropout = 0.2``, mosesvae.py:73-79) runs inside the step
kernels -- layer l+1 reads ``h^l * keep / (1 - p)`` -- with the keep mask generated on device by a counter-based hash from an explicit
seed (``forward(..., drop_seed=)``; by default drawn from torch's CPU generator, so ``torch.manual_seed`` makes a run reproducible) or
injected (``forward(..., drop_mask=)``: uint8 ``[layers-1, T, B, H]``; the parity tests inject the mask the reference drew).  ``eval()``
computes the deterministic network.  Under data parallelism (an initialised ``torch.distributed`` group) a TRAINING forward (train mode,
gradients enabled) takes the token mean of the reconstruction loss (mosesvae.py:193-197) over the GLOBAL number of non-pad targets
(``dp_global_token_mean``, one 4-byte all-reduce on ``dp_group``), so that the all-reduced gradient equals the single-process gradient of
the global batch; eval / no_grad forwards never communicate.

Against posterior collapse (additions, train mode only, off by default): ``word_dropout`` replaces the decoder's
input tokens by ``<unk>`` with that probability (never ``<bos>``, the last input token or padding; the encoder and the targets stay clean)
and ``free_bits`` makes ``kl_loss`` the objective ``sum_j max(m_j, free_bits)`` over the per-dimension batch means m_j of the KL, with
the KL itself in ``last_kl``.  With both at 0 the step issues exactly the launches it issues without them.
"""
import functools
import math
import os
import types

import torch
import torch.distributed as dist
import torch.nn as nn

from . import _lib as L
from . import ops
from .models import (LinearWeights, EmbeddingWeights, RNNWeights, _Workspace, _SavedState, _pad, _require_cuda, _LDPAD, _dyk, _grad_views, _kmajor_gemm,
                     _pack_rnn_stack, _gru_param_grads)
from .vocab import PaddedBatch, pad_batch, token_rows, length_order, smiles_token_table, smiles_chem_table, smiles_emit_table, SelfiesVocab, selfies_info_table


class _RowsWorkspace(_Workspace):
    """A _Workspace whose buffers are views of grow-only flat allocations, one per (name, row width, dtype, device): the passes of
    iw_log_likelihood, whose (rows, T) change from pass to pass, reuse one set of decoder buffers instead of allocating and zero-filling a
    new set per shape.  Every buffer of the teacher-forced decoder (_dec_forward) is an array of rows of a fixed width, and the columns
    that must stay zero (a leading dimension's padding, the unused gate slot of a [*, 4H] addend) are never written, so they stay zero
    under any row count; the rows themselves are written before they are read in every pass.  (Not for the encoder half: it reads slot 0
    of its hidden-state buffer as the zero initial state without writing it.)"""

    def get(self, name, shape, dtype, device):
        key, n = (name, shape[-1], dtype, device), math.prod(shape)
        b = self.bufs.get(key)
        if b is None or b.numel() < n:
            self.bufs[key] = None                                          # the smaller buffer goes before the larger one is allocated
            b = self.bufs[key] = torch.zeros(n, dtype=dtype, device=device)
        return b[:n].view(shape)


class ReLU(nn.Module):
    """Marker (fused into the producing GEMM's epilogue)."""


class SmilesReaders:
    """The methods that read token rows as SMILES molecules under ONE vocabulary: the syntax check, the graph walk and everything built on
    it.  ``VAE`` inherits them for its own vocabulary; ``SmilesView`` inherits them for another one (the SMILES rows a SELFIES model's
    samples decode to).  They ask of ``self`` exactly this: ``vocabulary``, ``bos`` / ``eos`` / ``pad``, ``device``, ``_rows(x, who, dev)``
    (the row intake) and ``_vocab_table(key, build, dev)`` (build(vocabulary), cached per device) -- and nothing else of a model, which
    is what lets the view stand in for one."""

    def _smiles_table(self, dev):
        return self._vocab_table("smi_tok", smiles_token_table, dev)

    _SMI_START = 0xFF << 16                  # the automaton's initial state word 0: mode START, depth 0, no previous token

    @torch.no_grad()
    def syntax_valid(self, x, bad_pos=False):
        """Which token rows are well-formed SMILES strings ending in <eos> (the automaton of sample(syntax=True), run over finished rows by
        mvae_smiles_syntax_check; syntax only, no chemistry).  x: padded ids [B, T] (bos first) on the device, or a list of id tensors
        (bos first) or strings.  Returns a bool [B] device tensor; bad_pos=True also returns int32 [B]: the index of the first refused
        token, T for a row without <eos>, -1 for a valid row."""
        dev = self.device
        _require_cuda(dev, "mosesvae.VAE.syntax_valid")
        x = self._rows(x, "syntax_valid", dev)
        B = x.shape[0]
        valid = torch.empty(B, dtype=torch.uint8, device=dev)
        bad = torch.empty(B, dtype=torch.int32, device=dev) if bad_pos else None
        ops.smiles_syntax_check(x, self._smiles_table(dev), self.eos, valid, bad)
        return (valid.bool(), bad) if bad_pos else valid.bool()

    def _smiles_chem_table(self, dev):
        return self._vocab_table("smi_chem", smiles_chem_table, dev)

    def _graph_rows(self, x, who):
        """syntax_valid's input handling, then one mvae_smiles_graph_rows launch: (status, bad_pos, desc, formula), int32, on the device."""
        dev = self.device
        _require_cuda(dev, "mosesvae.VAE." + who)
        if len(self.vocabulary) > 64:
            raise ValueError(f"{who}: the vocabulary has {len(self.vocabulary)} ids, at most 64 are supported")
        return ops.smiles_graph_rows(self._rows(x, who, dev), self._smiles_table(dev), self._smiles_chem_table(dev), self.eos)

    @torch.no_grad()
    def chem_valid(self, x, return_status=False, kekule=False):
        """Which token rows are well-formed AND valence-consistent SMILES strings (the graph walk of include/mvae.h, "SMILES graph", one
        mvae_smiles_graph_rows launch, no host wait): every atom within the largest valence its element and charge allow, no ring bond
        doubling an existing bond, every aromatic atom in a ring.  A necessary condition for chemical validity, not a sufficient one:
        nothing is kekulised.  x: what ``syntax_valid`` takes.  Returns a bool [B] device tensor; return_status=True also returns the
        int32 [B] status (ops.SMILES_STATUS_NAMES) and the int32 [B] bad_pos (the column of the first error, -1 for a row that is ok).
        ``kekule=True``: the answer is "status 0 under ``kekule``" instead -- valence-consistent and kekulisable, one
        mvae_smiles_kekule_rows launch; return_status=True then returns the status of ops.KEKULE_STATUS_NAMES alone, the kekule entry
        having no bad_pos.  Still a necessary condition only, and not rdkit's verdict."""
        if kekule:
            status = self.kekule(x, mate=False)["status"]
            return (status == 0, status) if return_status else status == 0
        status, bad, _, _ = self._graph_rows(x, "chem_valid")
        return (status == 0, status, bad) if return_status else status == 0

    @torch.no_grad()
    def kekule(self, x, mate=True):
        """The kekulisation test of token rows x (what ``syntax_valid`` takes), on the device, one mvae_smiles_kekule_rows launch, no
        host wait: {"status": int32 [B] (ops.KEKULE_STATUS_NAMES: ``chem_valid``'s status, or 7 where a valence-consistent row's aromatic
        atoms cannot all take their one ring double bond), "n_atoms", "n_bonds", "pairs", "deficiency": int32 [B] (the aromatic atoms
        that need a double bond, the aromatic ring bonds among them, the size of a maximum matching, the atoms it leaves over; zeros
        unless the status is 0 or 7), "mate": uint8 [B, 128] (the partner of atom a, in string order, in the matching found; 255: none),
        None with ``mate=False``}.  Status 0 is "kekulisable": tighter than valence-consistent, still necessary and not sufficient, with
        no aromaticity perception -- NOT rdkit's Kekulize or SanitizeMol (include/mvae.h, "Kekulisation").  ValueError for a vocabulary
        of more than 64 ids."""
        dev = self.device
        _require_cuda(dev, "mosesvae.VAE.kekule")
        if len(self.vocabulary) > 64:
            raise ValueError(f"kekule: the vocabulary has {len(self.vocabulary)} ids, at most 64 are supported")
        return ops.kekule_dict(*ops.smiles_kekule_rows(self._rows(x, "kekule", dev), self._smiles_table(dev), self._smiles_chem_table(dev),
                                                       self.eos, mate=None if mate else False))

    def _smiles_emit_table(self, dev):
        return self._vocab_table("smi_emit", smiles_emit_table, dev)

    @torch.no_grad()
    def respell(self, x, seed=0, draw=None, max_content=127):
        """A randomised respelling of token rows x (what ``syntax_valid`` takes) on the device, one mvae_smiles_rewrite_rows launch, no
        host wait: (rows int64 [B, max(T, max_content + 2)] -- <bos>, the new tokens, <eos>, <pad> --, status int32 [B],
        ops.REWRITE_STATUS_NAMES).  Row b is read into the walk's graph and written back from a random root in a random neighbour order,
        a pure function of (the row, seed, draw[b]); draw: integers [B] taken mod 2^32, None for the row numbers.  A row that cannot be
        respelled (status != 0: not well-formed or not valence-consistent, stereo tokens, a multiple bond that would close a ring, no
        free ring digit, more than 15 open branches, more than max_content tokens, a token the vocabulary lacks) comes back unchanged.
        The same graph under this library's walk; NOT a canonical SMILES and not rdkit's doRandom (include/mvae.h, "SMILES rewrite").
        ValueError for a vocabulary of more than 64 ids."""
        dev = self.device
        _require_cuda(dev, "mosesvae.VAE.respell")
        if len(self.vocabulary) > 64:
            raise ValueError(f"respell: the vocabulary has {len(self.vocabulary)} ids, at most 64 are supported")
        x = self._rows(x, "respell", dev)
        if draw is not None:
            draw = ops.draw_words(torch.as_tensor(draw).to(dev).reshape(-1))
            if draw.numel() != x.shape[0]:
                raise ValueError(f"respell: draw has {draw.numel()} entries, x has {x.shape[0]} rows")
        rows, _, status = ops.smiles_rewrite_rows(x, self._smiles_table(dev), self._smiles_chem_table(dev), self._smiles_emit_table(dev),
                                                  self.bos, self.eos, self.pad, seed, draw, max_content)
        return rows, status

    @torch.no_grad()
    def canonical(self, x, max_content=127, info=False):
        """The canonical spelling of token rows x (what ``syntax_valid`` takes) on the device, one mvae_smiles_canon_rows launch, no host
        wait: (rows int64 [B, max(T, max_content + 2)] -- <bos>, the new tokens, <eos>, <pad> --, status int32 [B],
        ops.REWRITE_STATUS_NAMES).  ``respell`` with the atoms ordered by a canonical rank instead of a hash: two spellings of one graph
        give one row, so rows can be compared as molecules by comparing tokens (include/mvae.h, "SMILES canon": equal rows always mean
        equal graphs; the converse is tested on every tie of the test corpus, not proved).  No aromaticity perception, no stereo, NOT
        rdkit's canonical SMILES.  A row that cannot be written (status != 0, ``respell``'s reasons) comes back unchanged.
        ``info=True`` also returns {"atoms", "first_classes", "rounds", "ties": int32 [B], "rank": uint8 [B, 128]}.  ValueError for a
        vocabulary of more than 64 ids."""
        dev = self.device
        _require_cuda(dev, "mosesvae.VAE.canonical")
        if len(self.vocabulary) > 64:
            raise ValueError(f"canonical: the vocabulary has {len(self.vocabulary)} ids, at most 64 are supported")
        x = self._rows(x, "canonical", dev)
        want = None if info else False
        rows, _, status, inf, rank = ops.smiles_canon_rows(x, self._smiles_table(dev), self._smiles_chem_table(dev), self._smiles_emit_table(dev),
                                                           self.bos, self.eos, self.pad, max_content, info=want, rank=want)
        if not info:
            return rows, status
        extra = {name: inf[:, i] for i, name in enumerate(ops.CANON_INFO)}
        extra["rank"] = rank
        return rows, status, extra

    @torch.no_grad()
    def normal_form(self, x, max_content=127, info=False):
        """The aromatic normal form of token rows x (what ``syntax_valid`` takes) on the device, one mvae_smiles_aromatize_rows launch,
        no host wait: (rows int64 [B, max(T, max_content + 2)] -- <bos>, the new tokens, <eos>, <pad> --, status int32 [B],
        ops.AROMATIZE_STATUS_NAMES).  ``canonical`` behind an aromaticity perception: the row's graph is read, the atoms on a cycle of
        5 - 7 candidate atoms with 4 k + 2 electrons get the aromatic flag, the bonds between them become aromatic bonds, and that graph
        is written in the canonical spelling, so that a Kekule spelling, an aromatic spelling and every respelling of one molecule are one
        row (include/mvae.h, "Aromatic normal form": this library's own rule, NOT rdkit's aromaticity model or canonical SMILES; no
        envelope cycles, no stereo).  A row that cannot be written (status != 0: ``canonical``'s reasons, 7: it does not kekulise, 17: a
        lower-case atom that the rule does not find aromatic) comes back unchanged.  ``info=True`` also returns {"atoms", "aromatic",
        "raised", "lowered_bonds": int32 [B], "arom": uint8 [B, 128]}.  ValueError for a vocabulary of more than 64 ids."""
        dev = self.device
        _require_cuda(dev, "mosesvae.VAE.normal_form")
        if len(self.vocabulary) > 64:
            raise ValueError(f"normal_form: the vocabulary has {len(self.vocabulary)} ids, at most 64 are supported")
        x = self._rows(x, "normal_form", dev)
        want = None if info else False
        rows, _, status, inf, arom = ops.smiles_aromatize_rows(x, self._smiles_table(dev), self._smiles_chem_table(dev),
                                                               self._smiles_emit_table(dev), self.bos, self.eos, self.pad, max_content,
                                                               info=want, arom=want)
        if not info:
            return rows, status
        extra = {name: inf[:, i] for i, name in enumerate(ops.AROMATIZE_INFO)}
        extra["arom"] = arom
        return rows, status, extra

    @torch.no_grad()
    def scaffold_smiles(self, x, max_content=127):
        """The Murcko scaffold of token rows x (what ``syntax_valid`` takes) as token rows on the device, one
        mvae_smiles_scaffold_smiles_rows launch, no host wait: (out int64 [B, max(T, max_content + 2)] -- <bos>, the scaffold's tokens,
        <eos>, <pad> --, out_len int32 [B], status int32 [B], ops.SCAFFOLD_SMILES_STATUS_NAMES).  The scaffold atoms of ``scaffolds``
        with every lost bond turned into hydrogens, in the spelling of ``canonical`` (include/mvae.h, "Scaffold SMILES"): rows that can
        be shown, handed to ``data.compile_substructures`` once decoded, and compared exactly.  A row without a scaffold (status != 0:
        ``canonical``'s reasons, or 14: no ring) is the EMPTY row <bos> <eos> with out_len 2, never a copy.  NOT rdkit's
        MurckoScaffoldSmiles: nothing is sanitised, no aromaticity perception, no stereo.  ValueError for a vocabulary of more than 64 ids."""
        dev = self.device
        _require_cuda(dev, "mosesvae.VAE.scaffold_smiles")
        if len(self.vocabulary) > 64:
            raise ValueError(f"scaffold_smiles: the vocabulary has {len(self.vocabulary)} ids, at most 64 are supported")
        x = self._rows(x, "scaffold_smiles", dev)
        out, out_len, status, _ = ops.smiles_scaffold_smiles_rows(x, self._smiles_table(dev), self._smiles_chem_table(dev),
                                                                  self._smiles_emit_table(dev), self.bos, self.eos, self.pad, max_content,
                                                                  info=False)
        return out, out_len, status

    def _substructure_words(self, x, table, max_steps=65536, map_query=None):
        """(status, hit, undecided[, map]) of one mvae_smiles_substruct_rows launch over token rows x on the device; table: a
        ``data.SubstructureTable``."""
        dev = self.device
        status, hit, undecided, emb, _ = ops.smiles_substruct_rows(x, self._smiles_table(dev), self._smiles_chem_table(dev), self.eos, table.on(dev),
                                                                   max_steps, map_query, steps=False)
        return (status, hit, undecided) if map_query is None else (status, hit, undecided, emb)

    @torch.no_grad()
    def has_substructure(self, x, patterns, max_steps=65536, return_map=None):
        """Which of the patterns (``data.compile_substructures``: 1 to 64 SMILES fragments, or a ``SubstructureTable`` to compile them
        once) the token rows x (what ``syntax_valid`` takes) contain, on the device, one mvae_smiles_substruct_rows launch, no host
        wait: (hit bool [B, Q], undecided bool [B, Q]).  hit[b, q]: the graph of row b contains pattern q -- an injective map of the
        pattern's atoms that keeps element, aromatic flag and charge of every atom and the class of every bond (include/mvae.h, "SMILES
        substructure"): graph containment, NOT SMARTS and not rdkit's HasSubstructMatch.  undecided[b, q]: the backtracking search
        examined ``max_steps`` candidates (1 to 2^20) without an answer; such a pair is neither hit nor miss.  A row the SMILES walk
        refuses contains nothing.  ``return_map=q`` also returns uint8 [B, 32]: the first (lexicographically smallest) embedding of
        pattern q, atom numbers of the row in the pattern's atom order, 0xFF beyond its atoms and where there is no hit.  ValueError
        for a refused pattern, a vocabulary of more than 64 ids, max_steps or return_map out of range."""
        from .data import compile_substructures
        dev = self.device
        _require_cuda(dev, "mosesvae.VAE.has_substructure")
        table = compile_substructures(patterns, self.vocabulary)
        x = self._rows(x, "has_substructure", dev)
        out = self._substructure_words(x, table, max_steps, return_map)
        hit, undecided = ops.substruct_bits(out[1], len(table)), ops.substruct_bits(out[2], len(table))
        return (hit, undecided) if return_map is None else (hit, undecided, out[3])

    @torch.no_grad()
    def descriptors(self, x):
        """The graph walk's figures for token rows x (what ``syntax_valid`` takes), a dict of device tensors -- one graph-walk launch, one matrix-vector product for the weight, no host wait:
        "status" and "bad_pos" as ``chem_valid`` returns them; "heavy_atoms", "bonds", "rings", "ring_atoms", "aromatic_atoms",
        "hydrogens", "charge", "hetero_atoms" (int32 [B]); "formula" (int32 [B, 11]: atoms per element of vocab.SMI_ELEMENTS, hydrogens
        first; ``data.formula_strings`` spells it); "weight" (float32 [B]: formula . vocab.ATOMIC_WEIGHTS).  Rows whose status is not 0
        have zeros everywhere."""
        return ops.graph_descriptors(*self._graph_rows(x, "descriptors"))

    @torch.no_grad()
    def fingerprints(self, x):
        """The circular fingerprint of token rows x (what ``syntax_valid`` takes): {"status": int32 [B], "fp": int64 [B, 16]} on the
        device, one mvae_smiles_fp_rows launch, no host wait.  1024 bits per row, radius 2, built like ECFP4 on the graph of the SMILES
        graph walk but NOT rdkit's Morgan fingerprint (include/mvae.h, "Circular fingerprint": nothing is kekulised, the bits are
        comparable within this library only); "status" is ``chem_valid``'s, and a row whose status is not 0 has an all-zero
        fingerprint.  ValueError for a vocabulary of more than 64 ids."""
        dev = self.device
        _require_cuda(dev, "mosesvae.VAE.fingerprints")
        if len(self.vocabulary) > 64:
            raise ValueError(f"fingerprints: the vocabulary has {len(self.vocabulary)} ids, at most 64 are supported")
        status, fp = ops.smiles_fp_rows(self._rows(x, "fingerprints", dev), self._smiles_table(dev), self._smiles_chem_table(dev), self.eos)
        return {"status": status, "fp": fp}

    @torch.no_grad()
    def tanimoto(self, x, y):
        """The Tanimoto similarity of the fingerprints of two batches, pair by pair: float32 [B] on the device, |a & b| / |a | b| as one
        f32 division, 0 where the union is empty (so 0 wherever a row is not ok).  x, y: what ``fingerprints`` takes, equally many
        rows (ValueError otherwise).  Two fingerprint launches and a few torch ops; the search over a corpus is
        ``MosesDeviceDataset.nearest_fingerprints``."""
        a, b = self.fingerprints(x)["fp"], self.fingerprints(y)["fp"]
        if a.shape[0] != b.shape[0]:
            raise ValueError(f"tanimoto: {a.shape[0]} rows against {b.shape[0]}")
        count = lambda t: ((t.view(torch.uint8)[:, :, None] >> torch.arange(8, device=t.device, dtype=torch.uint8)) & 1).sum((1, 2))
        c = count(a & b)
        u = count(a) + count(b) - c
        return torch.where(u > 0, c.float() / u.clamp(min=1).float(), torch.zeros((), device=a.device))

    @torch.no_grad()
    def scaffolds(self, x):
        """The Murcko scaffold and the graph keys of token rows x (what ``fingerprints`` takes), on the device, one
        mvae_smiles_scaffold_rows launch, no host wait: {"status": int32 [B], "mask": int64 [B, 2] (bit a of word a >> 6: atom a, in
        string order, is in the scaffold), "atoms", "bonds", "linker_atoms", "exo_atoms": int32 [B] (of the scaffold), "mol_key",
        "scaffold_key": int64 [B]}.  The scaffold is the ring atoms, the linkers between rings and the atoms double-bonded to either, on
        the graph of the SMILES graph walk -- NOT rdkit's MurckoScaffold; the keys are equal for equal graphs however the string spells
        them, ignore stereochemistry, and are no canonical SMILES (include/mvae.h, "Murcko scaffold", "Graph key").  A key of 0 means
        none: the row's status is not 0, or (scaffold key) it has no ring.  ValueError for a vocabulary of more than 64 ids."""
        dev = self.device
        _require_cuda(dev, "mosesvae.VAE.scaffolds")
        if len(self.vocabulary) > 64:
            raise ValueError(f"scaffolds: the vocabulary has {len(self.vocabulary)} ids, at most 64 are supported")
        return ops.scaffold_dict(*ops.smiles_scaffold_rows(self._rows(x, "scaffolds", dev), self._smiles_table(dev),
                                                           self._smiles_chem_table(dev), self.eos))

    @torch.no_grad()
    def fragments(self, x):
        """The fragments of token rows x (what ``fingerprints`` takes) and their graph keys, on the device, one
        mvae_smiles_fragment_rows launch, no host wait: {"status": int32 [B], "mask": int64 [B, 16, 2] (bit a of word a >> 6 of slot f:
        atom a, in string order, is in fragment f), "fragments", "cuts", "acyl_cuts", "largest": int32 [B], "keys": int64 [B, 16] (0 in
        unused slots)}.  A row is cut at the bonds between a ring and its substituents and at acyl-heteroatom bonds (amide, ester, ...),
        never at a terminal atom; the fragments are numbered by their lowest atom and keyed as ``scaffolds`` keys a scaffold
        (include/mvae.h, "Fragments").  This library's own rule: NOT BRICS, not RECAP, no agreement with a toolkit is claimed.  A row
        whose status is not 0 has zeros; one with more than 16 fragments has status ops.SMILES_STATUS_FRAG_MANY (15), zero mask and
        keys, and its true counts.  ValueError for a vocabulary of more than 64 ids."""
        dev = self.device
        _require_cuda(dev, "mosesvae.VAE.fragments")
        if len(self.vocabulary) > 64:
            raise ValueError(f"fragments: the vocabulary has {len(self.vocabulary)} ids, at most 64 are supported")
        return ops.fragment_dict(*ops.smiles_fragment_rows(self._rows(x, "fragments", dev), self._smiles_table(dev),
                                                           self._smiles_chem_table(dev), self.eos))

    @torch.no_grad()
    def fragment_smiles(self, x, frag=0, max_content=127):
        """Fragment number ``frag`` of token rows x (what ``syntax_valid`` takes) as token rows on the device, one
        mvae_smiles_fragment_smiles_rows launch, no host wait: (out int64 [B, max(T, max_content + 2)], out_len int32 [B], status int32
        [B], ops.FRAGMENT_SMILES_STATUS_NAMES).  The atoms of fragment ``frag`` of ``fragments`` with every lost bond turned into
        hydrogens, in the spelling of ``canonical`` (include/mvae.h, "Fragments"): rows that can be shown and handed to
        ``data.compile_substructures`` once decoded.  A row without that fragment (status != 0: ``canonical``'s reasons, or 16: fewer
        fragments) is the EMPTY row <bos> <eos> with out_len 2, never a copy.  NOT BRICS, not RECAP.  ValueError for a vocabulary of
        more than 64 ids or frag < 0."""
        dev = self.device
        _require_cuda(dev, "mosesvae.VAE.fragment_smiles")
        if len(self.vocabulary) > 64:
            raise ValueError(f"fragment_smiles: the vocabulary has {len(self.vocabulary)} ids, at most 64 are supported")
        x = self._rows(x, "fragment_smiles", dev)
        out, out_len, status, _ = ops.smiles_fragment_smiles_rows(x, self._smiles_table(dev), self._smiles_chem_table(dev),
                                                                  self._smiles_emit_table(dev), self.bos, self.eos, self.pad, frag, max_content,
                                                                  info=False)
        return out, out_len, status

    def edit_distance(self, x, y):
        """The token-level Levenshtein distance (unit costs for insert, delete and substitute, no transposition) between the rows of two
        batches, pair by pair: int32 [B] on the device, one launch (mvae_edit_distance_rows), no host wait.  x, y: padded ids [B, T] (bos
        first), or a list of id tensors (bos first) or of strings, under the model's vocabulary.  A row's content is what stands between
        <bos> and its first <eos> (or its last column); ids outside the vocabulary equal nothing.  ValueError, before any device work:
        batches of different sizes, a vocabulary of more than 64 ids, both sides wider than 129 columns."""
        x, y = self._rows(x, "edit_distance"), self._rows(y, "edit_distance")          # on the host: the checks come before any device work
        if x.shape[0] != y.shape[0]:
            raise ValueError(f"edit_distance: {x.shape[0]} rows against {y.shape[0]}")
        V = len(self.vocabulary)
        if V > ops.EDIT_V_MAX:
            raise ValueError(f"edit_distance: the vocabulary has {V} ids, at most {ops.EDIT_V_MAX} are supported")
        if min(x.shape[1], y.shape[1]) - 1 > ops.EDIT_PATTERN_MAX:
            raise ValueError(f"edit_distance: one side must have at most {ops.EDIT_PATTERN_MAX + 1} columns, got {x.shape[1]} and {y.shape[1]}")
        dev = self.device
        _require_cuda(dev, "mosesvae.VAE.edit_distance")
        return ops.edit_distance_rows(x.to(dev), y.to(dev), self.eos, V)


class VAE(_SavedState, SmilesReaders, nn.Module):
    def __init__(self, vocab, dtype=torch.bfloat16):
        super().__init__()
        q_d_h, q_n_layers, d_n_layers, d_dropout, d_z, d_d_h = 256, 1, 3, 0.2, 160, 512     # mosesvae.py:31-40
        self.vocabulary = vocab
        for ss in ("bos", "eos", "unk", "pad"):
            setattr(self, ss, getattr(vocab, ss))
        n_vocab, d_emb = len(vocab), vocab.vectors.size(1)
        if d_emb != n_vocab or vocab.vectors.size(0) != n_vocab:
            # the kernels fold the (identity-initialised, trainable) embedding into the layer-0 projections as a [V, V] table
            raise ValueError(f"mosesvae.VAE needs a one-hot vocabulary (vocab.vectors [{n_vocab}, {n_vocab}], mosesvae.py:48-50); "
                             f"got {tuple(vocab.vectors.shape)}")
        self.x_emb = EmbeddingWeights(n_vocab, d_emb)
        self.x_emb.padding_idx = self.pad
        self.x_emb.weight.data.copy_(vocab.vectors)                 # mosesvae.py:50 (overwrites the zeroed pad row too)
        self.encoder_rnn = RNNWeights("GRU", d_emb, q_d_h, q_n_layers)
        self.q_mu = nn.Sequential(LinearWeights(q_d_h, 256), ReLU(), LinearWeights(256, d_z))
        self.q_logvar = nn.Sequential(LinearWeights(q_d_h, 256), ReLU(), LinearWeights(256, d_z))
        self.decoder_rnn = RNNWeights("GRU", d_emb + d_z, d_d_h, d_n_layers)
        self.decoder_lat = LinearWeights(d_z, d_d_h)
        self.decoder_fc = LinearWeights(d_d_h, n_vocab)
        self.encoder = nn.ModuleList([self.x_emb, self.encoder_rnn, self.q_mu, self.q_logvar])
        self.decoder = nn.ModuleList([self.decoder_rnn, self.decoder_lat, self.decoder_fc])
        self.vae = nn.ModuleList([self.x_emb, self.encoder, self.decoder])
        self.d_z, self.d_dropout = d_z, d_dropout
        self.dp_global_token_mean = True     # DP: normalise the CE by the global non-pad token count (see module docstring)
        self.dp_force = False                # GradSync(force=True): make the token-count all-reduce even on a one-rank group (RCCL rehearsal)
        self.dp_group = None                 # process group of that reduction (None: the default group); moses_train_step sets it from the optimiser's GradSync
        self.last_drop_seed = None           # seed of the most recent train-mode forward (None: eval / injected mask)
        self.word_dropout = 0.0              # train mode: probability that a decoder INPUT token becomes <unk> (Bowman et al. 2016); 0 = off
        self.free_bits = 0.0                 # train mode: nats per latent dimension that cost nothing (Kingma et al. 2016, batch-mean form); 0 = off
        self.last_word_seed = None           # seed of the most recent word-dropout draw (None: off / injected mask)
        self.last_kl = None                  # free bits on: the KL itself of the most recent forward (device scalar; kl_loss is the objective)
        self.last_kl_per_dim = None          # free bits on: its per-dimension batch means [d_z] (device, detached)
        self.compute_dtype = dtype
        self.prior = "zeros"                 # sample_z_prior: "zeros" = the reference as written (mosesvae.py:211), "normal" = N(0, I) as its docstring says
        self.noise = "device"                # reparameterisation noise: "device" = drawn by the library inside the latent launch; "torch" = torch.randn on the device generator
        self.__dict__["noise_stream"] = ops.NoiseStream()
        self._init_saved_state()
        self.__dict__["_side"] = None

    def _side_stream(self, dev):
        return ops.side_stream(dev)

    @property
    def device(self):
        return next(self.parameters()).device

    def string2tensor(self, string, device="model"):
        ids = self.vocabulary.string2ids(string, add_bos=True, add_eos=True)
        return torch.tensor(ids, dtype=torch.long, device=self.device if device == "model" else device)

    def tensor2string(self, tensor):
        return self.vocabulary.ids2string(tensor.tolist(), rem_bos=True, rem_eos=True)

    def _seqs(self, x):
        """A list of strings and id tensors (bos first) as the list of int64 id tensors the reference passes around; strings on the host."""
        return [self.string2tensor(s, device="cpu") if isinstance(s, str) else torch.as_tensor(s, dtype=torch.long) for s in x]

    def _rows(self, x, who, dev=None):
        """vocab.token_rows under the model's vocabulary."""
        return token_rows(x, functools.partial(self.string2tensor, device="cpu"), self.pad, who, dev)

    # -- unique parameters in a fixed order (parameters() already de-duplicates the aliases)
    def _plist(self):
        return list(self.parameters())

    def _batch(self, x):
        """The reference's list of per-sequence LongTensors (sorted by length descending, as collate() yields them) or an already collated
        PaddedBatch -> (x_pad [B, T] int64, lengths [B] int32) on the model's device, one transfer."""
        dev = self.device
        if isinstance(x, PaddedBatch):                                # already collated into the kernels' layout (vocab.get_padded_collate_fn)
            return x.x_pad.to(dev, non_blocking=True), x.lengths.to(dev, non_blocking=True).to(torch.int32)
        b = pad_batch(list(x), self.pad)                              # padded where the tensors live (device tensors stay on the device)
        return b.x_pad.to(dev, non_blocking=True), b.lengths.to(dev, non_blocking=True)

    def _eps(self, B, eps):
        """The reparameterisation noise handed to the encoder node: the caller's tensor; None under noise == "device" (the library draws it
        inside the latent launch from self.noise_stream: an explicit seed + element counter, ops.NoiseStream); torch's device generator under
        noise == "torch" (mosesvae.py:159 as written: randn_like on the CUDA generator)."""
        if eps is not None:
            return eps.contiguous().float()
        if self.noise == "device":
            return None
        return torch.randn(B, self.d_z, device=self.device)

    def seed_noise(self, seed, counter=0):
        self.noise_stream.reseed(seed, counter)

    def _draw_drop(self, T, B, drop_mask, drop_seed):
        """Train mode: the decoder GRU's inter-layer dropout draw (nn.GRU(dropout=d_dropout if d_n_layers > 1 else 0)) as (p, seed, mask | None)."""
        NL = self.decoder_rnn.num_layers
        if not (self.training and self.d_dropout > 0 and NL > 1):
            return None
        if drop_mask is not None:
            m = torch.as_tensor(drop_mask).to(torch.uint8)
            if tuple(m.shape) != (NL - 1, T, B, self.decoder_rnn.hidden_size):
                raise ValueError(f"drop_mask must be [layers-1, T, B, H] = {(NL - 1, T, B, self.decoder_rnn.hidden_size)}, got {tuple(m.shape)}")
            self.last_drop_seed = None
            return (float(self.d_dropout), 0, m.contiguous().to(self.device))
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,))) if drop_seed is None else int(drop_seed)
        self.last_drop_seed = seed
        return (float(self.d_dropout), seed, None)

    def _collapse_opts(self):
        """(word_dropout, free_bits) as this forward applies them -- both 0.0 outside train mode --, after validating the attributes
        (ValueError, before any device work: a CPU model reports it too)."""
        p, fb = float(self.word_dropout), float(self.free_bits)
        if not (0.0 <= p < 1.0):                                       # (NaN fails both)
            raise ValueError(f"mosesvae.VAE.word_dropout must be in [0, 1), got {self.word_dropout}")
        if not (0.0 <= fb < math.inf):
            raise ValueError(f"mosesvae.VAE.free_bits must be finite and >= 0 (nats per latent dimension), got {self.free_bits}")
        return (p, fb) if self.training else (0.0, 0.0)

    def _word_drop(self, p, x_pad, len_t, word_mask, word_seed):
        """Train mode with word_dropout > 0: the decoder's input tokens, x_pad with the eligible positions (1 <= t <= len - 2: never <bos>,
        the last input token or padding) replaced by <unk> unless kept -- by word_mask [B, T] (1 = keep) when given, else by the counter
        hash of (seed, b * T + t) on the device (ops.dropout_keep_mask(seed, (B, T), p) restates it).  None when off: the decoder reads x_pad."""
        if p <= 0.0:
            self.last_word_seed = None
            return None
        B, T = x_pad.shape
        _require_cuda(x_pad.device, "mosesvae.VAE")
        mask, seed = None, 0
        if word_mask is not None:
            mask = torch.as_tensor(word_mask).to(torch.uint8)
            if tuple(mask.shape) != (B, T):
                raise ValueError(f"word_mask must be [B, T] = {(B, T)}, got {tuple(mask.shape)}")
            mask = mask.contiguous().to(x_pad.device)
            self.last_word_seed = None
        else:
            seed = int(torch.randint(0, 2 ** 31 - 1, (1,))) if word_seed is None else int(word_seed)
            self.last_word_seed = seed
        x_in = torch.empty_like(x_pad)
        ops.token_dropout(x_pad, len_t, x_in, B, T, self.unk, p, seed=seed, keep_mask=mask)
        return x_in

    def _note_kl(self, fb):
        """Free bits on: keep the KL itself and its per-dimension batch means beside the objective the forward returned as kl_loss."""
        if fb is None:
            self.last_kl = self.last_kl_per_dim = None
        else:
            self.last_kl, self.last_kl_per_dim = fb["kl2"][1].clone(), fb["kl_dim"].clone()

    def _dp_token_mean(self, recon, ntok):
        # Data-parallel TRAINING steps only (train mode, gradients enabled): every rank of `dp_group` makes this call once per step.  Evaluation,
        # no_grad encoding and rank-0-only validation stay collective-free (a collective only some ranks reach would deadlock).
        if (self.dp_global_token_mean and self.training and torch.is_grad_enabled() and dist.is_available() and dist.is_initialized()
                and (dist.get_world_size(self.dp_group) > 1 or self.dp_force)):
            # local mean = num_r / cnt_r; the gradient all-reduce averages over ranks, so scale to  num_r * world / sum_r cnt_r
            tot = ntok.detach().clone()
            dist.all_reduce(tot, group=self.dp_group)
            recon = recon * (ntok.detach() * dist.get_world_size(self.dp_group) / tot)
        return recon

    def _half_params(self, half):
        """(names, parameters) one half's autograd node owns: forward_encoder -> x_emb, encoder_rnn, q_mu, q_logvar; forward_decoder -> x_emb,
        decoder_rnn, decoder_lat, decoder_fc (the embedding feeds both GRUs)."""
        pre = ("x_emb.", "encoder_rnn.", "q_mu.", "q_logvar.") if half == "enc" else ("x_emb.", "decoder_rnn.", "decoder_lat.", "decoder_fc.")
        sel = [(n, p) for n, p in self.named_parameters() if n.startswith(pre)]
        return [n for n, _ in sel], [p for _, p in sel]

    def forward(self, x, eps=None, drop_mask=None, drop_seed=None, word_mask=None, word_seed=None):
        """x: list of LongTensors (one per sequence, sorted by length descending, as collate() yields them).
        Returns (kl_loss, recon_loss, z, logvar, x_padded, y) -- mosesvae.py:126-140 -- from ONE fused autograd node (the encoder and decoder
        halves of forward_encoder / forward_decoder, with the decoder's parameter gradients on a side stream beside the encoder's backward).
        eps / drop_mask / drop_seed inject the reparameterisation noise and the train-mode inter-layer dropout draw (parity tests).
        Train mode, additions against posterior collapse (both off by default):
          word_dropout > 0: the DECODER reads x with tokens replaced by <unk> (word_mask [B, T], 1 = keep, injects the draw; word_seed fixes
            the device draw; else a seed is drawn as drop_seed is and kept in last_word_seed).  The encoder, the cross-entropy targets and
            the returned x_padded stay the clean batch.
          free_bits > 0: kl_loss is the free-bits objective sum_j max(m_j, free_bits) over the per-dimension batch means m_j of this
            process's batch (under data parallelism: the rank's own; no collective), so `kl_weight * kl_loss + recon_loss` is the trained
            loss; the KL itself is in last_kl, the m_j in last_kl_per_dim (both None when free bits is off)."""
        wd, fb = self._collapse_opts()
        x_pad, len_t = self._batch(x)
        B, T = x_pad.shape
        eps = self._eps(B, eps)                                        # None: mosesvae.py:159's randn_like(mu) is drawn inside mvae_moses_latent_fwd
        drop = self._draw_drop(T, B, drop_mask, drop_seed)
        x_in = self._word_drop(wd, x_pad, len_t, word_mask, word_seed)
        if x_pad.is_cuda and torch.is_grad_enabled():
            self._side_stream(x_pad.device)                            # first use probes for a concurrent stream: here, not inside the backward
        opt = _opts(x_in, fb)
        kl, recon, z, logvar, y, ntok = _MosesFn.apply(self, x_pad, len_t, eps, drop, opt, *self._plist())
        self._note_kl(opt and opt["fb"])
        return kl, self._dp_token_mean(recon, ntok), z, logvar, x_pad, y

    def forward_encoder(self, x, eps=None):
        """mosesvae.py:142-164: x -> (z, kl_loss, logvar).  Runs the encoder half only (GRU(256), heads, reparameterisation + KL); differentiable
        w.r.t. x_emb / encoder_rnn / q_mu / q_logvar.  Train mode with free_bits > 0: kl_loss is the free-bits objective, as in `forward`."""
        _, fb = self._collapse_opts()
        x_pad, len_t = self._batch(x)
        _, params = self._half_params("enc")
        opt = _opts(None, fb)
        out = _MosesEncFn.apply(self, x_pad, len_t, self._eps(x_pad.shape[0], eps), opt, *params)
        self._note_kl(opt and opt["fb"])
        return out

    @torch.no_grad()
    def encode(self, x):
        """The posterior of every sequence of x (what forward_encoder takes: a list of id tensors sorted by length descending, or a
        PaddedBatch): (mu, logvar), float32 [B, d_z] on the device, in the order of x.  forward_encoder with eps = 0, so that z = mu; runs
        without gradients and in eval mode for the call (the training flag is restored)."""
        was_training = self.training
        self.eval()
        try:
            B = len(x)
            z, _, logvar = self.forward_encoder(x, eps=torch.zeros(B, self.d_z, device=self.device))
        finally:
            self.train(was_training)
        return z.float(), logvar.float()

    def forward_decoder(self, x, z, drop_mask=None, drop_seed=None, word_mask=None, word_seed=None):
        """mosesvae.py:166-199: teacher-forced decoder on the caller's latent z [B, d_z] -> (recon_loss, x_padded, y); differentiable w.r.t. z
        and x_emb / decoder_rnn / decoder_lat / decoder_fc.  Train mode applies the inter-layer dropout and the word dropout as `forward` does."""
        wd, _ = self._collapse_opts()
        x_pad, len_t = self._batch(x)
        B, T = x_pad.shape
        if tuple(z.shape) != (B, self.d_z):
            raise ValueError(f"forward_decoder: z must be [{B}, {self.d_z}], got {tuple(z.shape)}")
        drop = self._draw_drop(T, B, drop_mask, drop_seed)
        x_in = self._word_drop(wd, x_pad, len_t, word_mask, word_seed)
        _, params = self._half_params("dec")
        recon, y, ntok = _MosesDecFn.apply(self, x_pad, len_t, z.to(self.device), drop, _opts(x_in, 0.0), *params)
        return self._dp_token_mean(recon, ntok), x_pad, y

    def sample_z_prior(self, n_batch, normal=None):
        """mosesvae.py:200-211.  The reference AS WRITTEN returns zeros (its randn line is commented out, :207-210) although its docstring says
        z ~ N(0, I); a drop-in keeps that: `self.prior == "zeros"` (the default).  `normal=True` / `self.prior = "normal"` gives the documented
        N(0, I) draw -- from the library's counter hash (noise == "device") or torch's device generator."""
        if not (self.prior == "normal" if normal is None else normal):
            return torch.zeros((n_batch, self.d_z), device=self.device)
        if self.noise == "device" and self.device.type == "cuda":
            seed, off = self.noise_stream.take(n_batch * self.d_z)
            return ops.normal_fill(torch.empty(n_batch, self.d_z, device=self.device), 1.0, seed, off)
        return torch.randn(n_batch, self.d_z, device=self.device)

    @torch.no_grad()
    def sample(self, n_batch, max_len=100, z=None, temp=1.0, return_tokens=False, seed=None, top_k=None, top_p=None, return_logp=False,
               syntax=False, prefix=None):
        """mosesvae.py:214-262 (autoregressive decoding, multinomial sampling at temperature `temp`) on the GRU step kernels: per generated token
        one wavefront pass of the 3-layer stack (T = 1) and ONE sampling launch (head GEMV + softmax + multinomial + eos / end-pad bookkeeping +
        the next token's input rows: mvae_moses_sample_step) -- 4 launches per token, no torch arithmetic in the loop.  Randomness is explicit:
        `seed` (default: drawn from torch's CPU generator, so torch.manual_seed makes a run reproducible) feeds a counter hash of (step, row).
        Upstream bugs fixed: boolean masks, a real d_z.  Returns (list of strings, z).
        Additions beyond the reference: `top_k` keeps the k most probable tokens of each step, `top_p` the shortest most-probable-first prefix
        whose probability reaches top_p (ties by token id; both look at the unfiltered softmax(y / temp), and the draw is from their
        intersection, renormalised); None, top_k >= V and top_p >= 1 switch a filter off.  `return_logp=True` appends a third return value
        logq, float32 [B] on the device: the summed log-probability of tokens 1 .. end under the distribution they were drawn from,
        temperature and truncation included (at temp = 1 with the filters off that is log p(x | z) as `decode` reports it: an emitted `pad`
        token counts, unlike in `score`).  With a filter or return_logp the sampling launch is mvae_moses_sample_filtered_step (still 4
        launches per token); without them the method runs the launches it always ran.  The same seed gives the same tokens either way.
        `syntax=True` (an addition) constrains every step to the tokens that keep the string a well-formed SMILES
        string that can still be finished within max_len: balanced branches, closed rings and brackets, no dangling bond, a conservative
        bracket-atom grammar -- syntax only, valence and aromaticity stay unchecked.  The mask sits in front of the softmax inside the
        sampling launch (mvae_moses_sample_syntax_step, still 4 launches per token); top_k / top_p then act on the legal tokens and logq
        is that of the constrained distribution.  Every row then ends in <eos>.  Needs max_len >= 3 (ValueError) and a vocabulary with an
        atom token.
        `prefix` (an addition) keeps a fragment and lets the model finish the string: the tokens that follow <bos>,
        as one string or 1-D id tensor (without <bos> / <eos>) for every row, or a list of n_batch of them (an empty entry leaves its row
        unconstrained).  Row b writes its P_b prefix tokens at steps 1 .. P_b -- no temperature, filter or mask, no random draw consumed --
        and steps P_b + 1 .. run as they always do, inside the same launches (mvae_moses_sample_forced_step, still 4 launches per token).
        logq is then the log-probability of the FREE tokens given the prefix (a forced token adds nothing); `score` gives log p of the
        whole string.  The draw of a free step depends on (seed, step, row) alone, so a sample replayed with its own leading tokens as the
        prefix returns the same row, bit for bit.  ValueError, before any device work: a list of another length than n_batch, a character
        outside the vocabulary, an id outside [0, V) or one of <bos> / <eos> / <pad>, more than max_len - 2 prefix tokens.  With
        syntax=True the prefixes are walked by the automaton first (mvae_smiles_prefix_state, one host synchronisation before the loop):
        ValueError names the first row and position whose token it refuses, or whose prefix leaves too little room to finish the string
        within max_len; every row is then well-formed and ends in <eos>, prefix included.  prefix=None runs the launches it always ran."""
        top_k, top_p = self._check_filters(top_k, top_p)
        if syntax:
            self._check_syntax(max_len)
        forced = self._prefix_table(prefix, n_batch, max_len, "sample")
        dev = self.device
        _require_cuda(dev, "mosesvae.VAE.sample")
        if z is None:
            z = self.sample_z_prior(n_batch)
        if seed is None:
            seed = int(torch.randint(0, 2 ** 31 - 1, (1,)))
        filtered = top_k > 0 or top_p < 1.0 or return_logp
        x, end_pads, logq, _ = self._sample_tokens(z[:n_batch], max_len, temp, seed, top_k, top_p, filtered=filtered, syntax=syntax, forced=forced)
        xs, ends = x.cpu(), end_pads.cpu()
        if return_tokens:                                                # raw id tensors (specials included), for tests / downstream scoring
            out = [xs[b, :ends[b]] for b in range(n_batch)]
        else:
            out = [self.tensor2string(xs[b, :ends[b]]) for b in range(n_batch)]
        z = z.to(dev).float().contiguous()
        return (out, z, logq) if return_logp else (out, z)

    def _check_filters(self, top_k, top_p):
        """sample()'s top_k / top_p as the kernel takes them: (top_k, 0 = off; top_p, 1.0 = off).  ValueError for top_k < 1, top_p <= 0 / NaN."""
        V = self.x_emb.num_embeddings
        if top_k is None:
            k = 0
        else:
            k = int(top_k)
            if k < 1 or k != top_k:
                raise ValueError(f"sample: top_k must be an integer >= 1 (or None), got {top_k}")
            k = 0 if k >= V else k
        if top_p is None:
            p = 1.0
        else:
            p = float(top_p)
            if not p > 0.0:
                raise ValueError(f"sample: top_p must be in (0, 1] (or None), got {top_p}")
            p = min(p, 1.0)
        return k, p

    def _check_syntax(self, max_len):
        """syntax=True needs max_len >= 3 (<bos>, one atom, <eos>) and a vocabulary the automaton can write an atom with: ValueError
        otherwise, before any device work (a CPU model reports it too)."""
        if int(max_len) < 3:
            raise ValueError(f"sample / decode: syntax=True needs max_len >= 3 (<bos>, an atom, <eos>), got {max_len}")
        if isinstance(self.vocabulary, SelfiesVocab):
            raise ValueError("sample / decode: syntax=True constrains SMILES tokens and this model's vocabulary is a SelfiesVocab: every "
                             "SELFIES row is a molecule already; sample without syntax= and turn the rows into SMILES with VAE.to_smiles")
        self._smiles_table(None)

    def _prefix_table(self, prefix, n, max_len, what):
        """`prefix` of sample / decode / moses_generate as the forced launches take it: None for None, else (table, lens) on the host --
        table int32 [n, max_len] ([1, max_len] for one prefix broadcast to all rows), table[b, 1 : 1 + P_b] = the prefix ids and -1 (free)
        everywhere else, step 0 (<bos>) included; lens int32 [n] or [1] = P_b.  Raises the ValueErrors of the docstrings, before any
        device work."""
        if prefix is None:
            return None
        V, max_len = self.x_emb.num_embeddings, int(max_len)
        if isinstance(prefix, str) or torch.is_tensor(prefix):
            entries = [prefix]
        else:
            entries = list(prefix)
            if len(entries) != n:
                raise ValueError(f"{what}: prefix must be one string / id tensor or a list of {n} of them, got {len(entries)}")
        table = torch.full((len(entries), max(max_len, 1)), -1, dtype=torch.int32)
        lens = torch.zeros(len(entries), dtype=torch.int32)
        for b, e in enumerate(entries):
            if isinstance(e, str):
                if isinstance(self.vocabulary, SelfiesVocab):
                    bad = [sym for sym in self.vocabulary.split(e) if sym not in self.vocabulary.sym2char]
                else:
                    bad = [ch for ch in e if ch not in self.vocabulary.c2i]
                if bad:
                    raise ValueError(f"{what}: prefix of row {b}: character {bad[0]!r} is not in the vocabulary")
                ids = self.vocabulary.string2ids(e)
            else:
                t = torch.as_tensor(e)
                if t.dim() != 1 or t.dtype.is_floating_point or t.dtype == torch.bool:
                    raise ValueError(f"{what}: prefix of row {b} must be a string or a 1-D integer id tensor, got {tuple(t.shape)} {t.dtype}")
                ids = [int(i) for i in t.tolist()]
            for pos, i in enumerate(ids):
                if not 0 <= i < V or i in (self.bos, self.eos, self.pad):
                    raise ValueError(f"{what}: prefix of row {b}, position {pos}: id {i} is outside [0, {V}) or one of <bos> / <eos> / <pad>")
            if len(ids) > max(max_len - 2, 0):
                raise ValueError(f"{what}: prefix of row {b} has {len(ids)} tokens, max_len = {max_len} leaves room for {max(max_len - 2, 0)} "
                                 f"(<bos> and one more token are needed)")
            if ids:
                table[b, 1:1 + len(ids)] = torch.tensor(ids, dtype=torch.int32)
                lens[b] = len(ids)
        return table, lens

    def _check_prefix_syntax(self, forced, max_len, what):
        """The automaton over the prefixes of _prefix_table's (table, lens), all rows at once: one mvae_smiles_prefix_state launch and one
        host synchronisation.  ValueError naming the first row and position whose token the automaton refuses, or whose prefix leaves too
        few steps to finish the string within max_len."""
        table, lens = forced
        dev = self.device
        _require_cuda(dev, "mosesvae.VAE." + what)
        n, max_len = table.shape[0], int(max_len)
        state = torch.empty((n, 2), dtype=torch.int32, device=dev)
        res = torch.empty((2, n), dtype=torch.int32, device=dev)                  # need, bad_pos
        ops.smiles_prefix_state(table.to(dev)[:, 1:], lens.to(dev), self._smiles_table(dev), state, res[0], res[1])
        res = res.cpu()
        wrong = torch.nonzero((res[1] >= 0) | (res[0] > max_len - 1 - lens))
        if wrong.numel():
            b = int(wrong[0])
            need, bad, P = int(res[0, b]), int(res[1, b]), int(lens[b])
            if bad >= 0:
                raise ValueError(f"{what}: syntax=True: prefix of row {b}, position {bad}: token "
                                 f"{self.vocabulary.id2char(int(table[b, 1 + bad]))!r} is refused by the SMILES automaton")
            raise ValueError(f"{what}: syntax=True: prefix of row {b}, position {P}: the string needs {need} more tokens "
                             f"(<eos> included), max_len = {max_len} leaves {max_len - 1 - P}")

    def _forced_rows(self, forced, B, max_len, dev, what):
        """_prefix_table's (table, lens) on the device as int32 [B, max_len] (a broadcast prefix expanded)."""
        table = forced[0]
        if table.shape[0] not in (1, B) or table.shape[1] != max_len:
            raise ValueError(f"{what}: the prefix table is {tuple(table.shape)}, the batch needs [{B}, {max_len}]")
        return table.to(dev).expand(B, -1).contiguous()

    def _vocab_table(self, key, build, dev):
        """build(vocabulary): made once per model on the host (dev None), its device copy cached in the pack."""
        host = self.__dict__.get("_" + key)
        if host is None:
            host = self.__dict__["_" + key] = build(self.vocabulary)
        if dev is None:
            return host
        P = self._pack(dev)
        if key not in P:
            P[key] = host.to(dev)
        return P[key]

    @torch.no_grad()
    def to_smiles(self, x, smiles_vocab, normal=False, max_content=127, info=False):
        """SELFIES token rows x of a model built on a ``vocab.SelfiesVocab`` (padded ids [B, T], bos first, or a list of id tensors or
        SELFIES texts) as SMILES token rows in `smiles_vocab`, on the device, one mvae_selfies_decode_rows launch, no host wait: (rows
        int64 [B, max(T, max_content + 2)] -- <bos>, the tokens, <eos>, <pad> --, status int32 [B], ops.SELFIES_STATUS_NAMES).  Every row
        is derived into a graph by this library's own SELFIES rules (include/mvae.h, "SELFIES"; NOT the selfies package's decoder:
        agreement with it is neither tested nor claimed) and written in the canonical Kekule spelling of ``canonical``; a row that cannot
        be written (status 1: a token that is no symbol, or no atom; 9 - 13: the writer's reasons) gives the EMPTY row.  ``normal=True``
        runs mvae_smiles_aromatize_rows behind it: the rows are the aromatic normal form (``normal_form``), and the status of a decoded
        row that launch refuses is the launch's.  ``info=True`` also returns {"atoms", "ring_bonds", "reparented", "bad_column": int32
        [B]}.  ValueError for a model whose vocabulary is no SelfiesVocab and for a vocabulary of more than 64 ids."""
        if not isinstance(self.vocabulary, SelfiesVocab):
            raise ValueError("to_smiles: the model's vocabulary is no SelfiesVocab; its rows are SMILES rows already")
        if len(self.vocabulary) > 64 or len(smiles_vocab) > 64:
            raise ValueError(f"to_smiles: the vocabularies have {len(self.vocabulary)} and {len(smiles_vocab)} ids, at most 64 are supported")
        dev = self.device
        _require_cuda(dev, "mosesvae.VAE.to_smiles")
        x = self._rows(x, "to_smiles", dev)
        P = self._pack(dev)
        key = ("to_smiles", id(smiles_vocab))
        if key not in P:
            P[key] = (smiles_vocab, smiles_token_table(smiles_vocab).to(dev), smiles_chem_table(smiles_vocab).to(dev),
                      smiles_emit_table(smiles_vocab).to(dev))
        _, tok, chem, emit = P[key]
        v = smiles_vocab
        rows, _, status, inf = ops.selfies_decode_rows(x, self._vocab_table("selfies_info", selfies_info_table, dev), emit, v.bos, v.eos, v.pad,
                                                       max_content, info=None if info else False)
        if normal:
            rows, _, st2, _, _ = ops.smiles_aromatize_rows(rows, tok, chem, emit, v.bos, v.eos, v.pad, max_content, info=False, arom=False)
            status = torch.where(status == 0, st2, status)
        if not info:
            return rows, status
        return rows, status, {name: inf[:, i] for i, name in enumerate(ops.SELFIES_DECODE_INFO)}

    def _decode_setup(self, z, n_mol, pre, max_len, syntax, forced, who, check_prefix=True):
        """What _sample_tokens and _beam_search do in front of their token loops, for the rows of z (fp32 [rows, d_z] on the device: one
        per sample, or one per beam with each molecule's latent repeated) in workspace buffers named pre + ...: the initial state from
        decoder_lat, the 4-slot copies tbl4 / zp4 of the layer-0 addends, state [layers, 2, rows, ldh] (half 0 = h0 in every layer) with
        gates / hstate / add, the automaton's tok_info / gstate (syntax; else None), the device prefix table ftab (forced =
        _prefix_table's result for n_mol molecules, checked by the automaton first under syntax and check_prefix; else None) and the
        <bos> input rows gathered into add.  rnn[c] is the bound GRU pass that reads state half c and writes half 1 - c, h_top[c] the top
        layer's state in half c.  Uploading the prefix table waits for the device, so the callers allocate their own buffers before this
        call and nothing but the gather follows the upload."""
        dev = self.device
        P = self._pack(dev)
        ws, dt, f32 = self._ws, self.compute_dtype, torch.float32
        R, V, dz = z.shape[0], self.x_emb.num_embeddings, self.d_z
        pd = P["dec"]; Hd = pd["H"]; NL = self.decoder_rnn.num_layers
        Vp, ldh = _pad(V, 4), Hd + _LDPAD
        W = lambda name, shape, d=f32: ws.get(pre + name, shape, d, dev)
        h0 = W("h0", (R, Hd)); ops.gemm_nt(z, self.decoder_lat.weight, h0, R, Hd, dz, bias=self.decoder_lat.bias)
        tbl3 = W("tbl3", (V, 3 * Hd)); ops.gemm_nt(P["E_p"], pd["Wx_p"], tbl3, V, 3 * Hd, Vp)
        tbl4 = W("tbl4", (V, 4 * Hd)); tbl4[:, :3 * Hd].copy_(tbl3)
        zp3 = W("zp3", (R, 3 * Hd)); ops.gemm_nt(z, P["Wz"], zp3, R, 3 * Hd, dz)
        zp4 = W("zp4", (R, 4 * Hd)); zp4[:, :3 * Hd].copy_(zp3)
        state = W("state", (NL, 2, R, ldh), dt)            # [l][c] = the state a GRU step reads (c = 0 first), [l][1 - c] = the state it writes
        for l in range(NL):
            ops.cast_transpose(h0, R, Hd, dst=state[l][0])
        gates = [W(f"gates{l}", (1, R, 4 * Hd), dt) for l in range(NL)]
        hstate = [W(f"hstate{l}", (2, R, Hd)) for l in range(NL)]
        add = W("add", (1, R, 4 * Hd))
        w = torch.full((R, 1), self.bos, dtype=torch.long, device=dev)
        halves = [h.unbind(0) for h in state.unbind(1)]                  # [c][l] = layer l's [R, ldh] state in half c (at T = 1 also its output)
        ldws = [pd["ldw"]] * NL
        rnn = [functools.partial(ops.rnn_fwd, L.CELL_GRU, dt, 1, R, Hd, add, 0, pd["Wih"], ldws, pd["Whh"], ldws, pd["bias"], halves[1 - c], ldh,
                                 None, gates, hstate, h0=halves[c], ldh0=ldh, persist=False) for c in (0, 1)]
        tok_info = gstate = ftab = None
        if syntax:
            tok_info = self._smiles_table(dev)
            gstate = torch.zeros((R, 2), dtype=torch.int32, device=dev)
            gstate[:, 0] = self._SMI_START
        if forced is not None:
            if syntax and check_prefix:
                self._check_prefix_syntax(forced, max_len, who)
            ftab = self._forced_rows(forced, n_mol, max_len, dev, who)
        ops.gather_rows_tb(w, tbl4, add, R, 1, V, 4 * Hd, base=zp4)      # the <bos> input rows; later ones come out of the loop's own launch
        return types.SimpleNamespace(tbl4=tbl4, zp4=zp4, add=add, state=state, h_top=(halves[0][-1], halves[1][-1]), rnn=rnn, w=w,
                                     tok_info=tok_info, gstate=gstate, ftab=ftab,
                                     w_fc=P["Wfc"], b_fc=self.decoder_fc.bias, ldh=ldh, V=V, H=Hd)

    _FNV_BASIS = -3750763034362895579       # 0xcbf29ce484222325, the 64-bit FNV-1a offset basis, as an int64

    def _sample_tokens(self, z, max_len, temp, seed, top_k=0, top_p=1.0, filtered=True, syntax=False, forced=None, check_prefix=True):
        """The sampling loop without the host side: (x [B, max_len] int64 -- bos first, pad after each end --, ends [B] int64, logq [B] fp32,
        hash [B] int64: FNV-1a over x[b, 1 : end]) on the device.  top_k (0: off) / top_p (1.0: off) as _check_filters returns them.
        filtered=False issues mvae_moses_sample_step instead (sample()'s default path) and returns None for logq and hash.  syntax=True
        issues mvae_moses_sample_syntax_step (the filtered launch under the SMILES automaton; filtered is then implied).  forced
        (_prefix_table's result, rows for this batch) issues mvae_moses_sample_forced_step in place of any of the three: the rows write
        their prefix tokens first; logq and hash stay None with filtered=False.  With syntax the prefixes are walked by the automaton
        first (_check_prefix_syntax) unless the caller has done so for all its batches (check_prefix=False)."""
        if syntax:
            self._check_syntax(max_len)
            filtered = True                                               # logq and hash come with it
        dev = self.device
        _require_cuda(dev, "mosesvae.VAE.sample")
        z = z.to(dev).float().contiguous()
        B = z.shape[0]
        x = torch.full((B, max_len), self.pad, dtype=torch.long, device=dev)
        x[:, 0] = self.bos
        end_pads = torch.full((B,), max_len, dtype=torch.long, device=dev)
        eos_mask = torch.zeros(B, dtype=torch.uint8, device=dev)
        logq = hsh = None
        if filtered:
            logq = torch.zeros(B, dtype=torch.float32, device=dev)
            hsh = torch.full((B,), self._FNV_BASIS, dtype=torch.long, device=dev)
        d = self._decode_setup(z, B, "smp_", max_len, syntax, forced, "sample", check_prefix)
        launch, tail = ops.moses_sample_step, {}
        if filtered or forced is not None:
            launch, tail = ops.moses_sample_filtered_step, dict(top_k=top_k, top_p=top_p, logq=logq, hash=hsh)
        if syntax:
            launch = ops.moses_sample_syntax_step
            tail.update(tok_info=d.tok_info, gstate=d.gstate, max_len=max_len)
        if forced is not None:
            launch = ops.moses_sample_forced_step
            tail.update(forced=d.ftab, max_len=max_len)
        step = functools.partial(launch, ldh=d.ldh, w_fc=d.w_fc, bias=d.b_fc, temp=temp, seed=seed, eos_id=self.eos, table=d.tbl4, base=d.zp4,
                                 add_out=d.add, x=x, end_pads=end_pads, eos_mask=eos_mask, w_out=d.w, B=B, V=d.V, H=d.H, **tail)
        rnn, h_top = d.rnn, d.h_top
        cur = 0                                                           # the half the GRU step reads (swapped every token)
        for i in range(1, max_len):
            rnn[cur]()
            step(h_top[1 - cur], step=i)
            cur = 1 - cur
        return x, end_pads, logq, hsh

    @torch.no_grad()
    def decode(self, z, beam_width=1, max_len=100, return_tokens=False, syntax=False, prefix=None):
        """Deterministic decoding of the latents z [B, d_z] by beam search (an addition: the reference only samples); beam_width=1 is greedy
        decoding.  The `sample()` loop with the beam launch in place of the sampling launch: per generated token one wavefront pass of the
        3-layer stack (T = 1) and ONE mvae_moses_beam_step launch, which also reorders the recurrent state to the surviving beams -- 4 launches
        per token, no torch arithmetic and no host synchronisation in the loop; it runs to max_len as `sample` does.  A hypothesis' score is
        its raw summed log-probability log p(tokens 1..end | z) (no length normalisation; the `pad` steps after <eos> add nothing); ties
        are broken by (parent beam, token id), so a decode is deterministic.  Dropout is never applied.
        Returns (best string per molecule, scores [B]); return_tokens=True: (per molecule, its beam_width id tensors cut at their ends --
        bos first, <eos> last when it came -- best first, scores [B, beam_width]).
        `syntax=True` (an addition) searches over well-formed SMILES strings only: the automaton of
        sample(syntax=True) runs inside the beam launch (mvae_moses_beam_syntax_step, still 4 launches per token), and a beam proposes only
        the tokens that keep its string well-formed and finishable within max_len.  The score is NOT renormalised over the allowed tokens:
        it stays the model's log p(tokens | z) over all V classes -- the mask only removes candidates --, so `score` agrees with it and the
        search returns the most probable well-formed strings the beam finds (sampling renormalises because it defines a distribution;
        decoding does not).  Every returned string is then well-formed and ends in <eos> within max_len.  A molecule can have fewer than
        beam_width well-formed continuations (beam_width = 16 at max_len = 3): with return_tokens=True a hypothesis whose score is -inf
        is dead -- its tokens mean nothing -- and should be dropped by the caller; the best hypothesis is always finite.  Needs
        max_len >= 3 (ValueError) and a vocabulary with an atom token.  syntax=False runs the launches it always ran.
        `prefix` (an addition) searches the completions of a fragment: one prefix for every molecule or a list of
        B of them, in the forms and with the ValueErrors of `sample(prefix=)`.  At steps 1 .. P_b every live beam of molecule b proposes
        exactly one candidate, the prefix token, at score + log p(token) (mvae_moses_beam_forced_step, still 4 launches per token): the
        scores stay log p(tokens | z) of the whole string, prefix included, so `score` keeps agreeing with them; beams 1 .. K-1 stay dead
        through the prefix and come alive at the first free step.  With syntax=True the prefixes are checked by the automaton before the
        loop as in `sample`.  prefix=None runs the launches it always ran."""
        ids, ends, scores = self._beam_search(z, beam_width, max_len, syntax=syntax, prefix=prefix)
        xs, es = ids.cpu(), ends.cpu()
        B, K = es.shape
        if return_tokens:
            return [[xs[b, k, :es[b, k]] for k in range(K)] for b in range(B)], scores
        best, n = xs[:, 0].tolist(), es[:, 0].tolist()        # Python lists: per-row tensor indexing costs ~10 us a molecule
        return [self.vocabulary.ids2string(best[b][:n[b]], rem_bos=True, rem_eos=True) for b in range(B)], scores[:, 0]

    def _beam_search(self, z, beam_width, max_len, syntax=False, prefix=None):
        """decode() without the host side: (ids [B, K, max_len] int64, ends [B, K] int64, scores [B, K] fp32) on the device, best first.
        syntax=True issues mvae_moses_beam_syntax_step instead of mvae_moses_beam_step: every hypothesis with a finite score is a
        well-formed SMILES string ending in <eos>; the scores stay log p(tokens | z) (no renormalisation); a score of -inf marks a dead
        slot (fewer than K well-formed candidates), sorted last.  prefix (decode's) issues mvae_moses_beam_forced_step in place of either."""
        if syntax:
            self._check_syntax(max_len)
        V, dz = self.x_emb.num_embeddings, self.d_z
        K = int(beam_width)
        if not (1 <= K <= 16) or K > V:
            raise ValueError(f"decode: beam_width must be in [1, min(16, V = {V})], got {beam_width}")
        if int(max_len) < 1:
            raise ValueError(f"decode: max_len must be >= 1, got {max_len}")
        if z.dim() != 2 or z.shape[1] != dz or z.shape[0] < 1:
            raise ValueError(f"decode: z must be [B, {dz}], got {tuple(z.shape)}")
        forced = self._prefix_table(prefix, z.shape[0], max_len, "decode")
        dev = self.device
        _require_cuda(dev, "mosesvae.VAE.decode")
        max_len = int(max_len)
        B = z.shape[0]; R = B * K
        zr = z.to(dev).float().repeat_interleave(K, 0).contiguous()              # beams of molecule m: rows m*K .. m*K + K-1
        score = torch.full((B, K), float("-inf"), device=dev); score[:, 0] = 0.0    # beams 1..K-1 start dead: no duplicates at step 1
        score = score.view(R)
        fin = torch.zeros(R, dtype=torch.uint8, device=dev)
        ends = torch.full((R,), max_len, dtype=torch.long, device=dev)
        hist_tok = torch.empty((max_len, R), dtype=torch.int32, device=dev)          # row 0 (bos) is never read
        hist_par = torch.empty((max_len, R), dtype=torch.int32, device=dev)
        d = self._decode_setup(zr, B, "bm_", max_len, syntax, forced, "decode")
        launch, tail = ops.moses_beam_step, {}
        if syntax:
            launch, tail = ops.moses_beam_syntax_step, dict(tok_info=d.tok_info, gstate=d.gstate, max_len=max_len)
        if forced is not None:
            launch = ops.moses_beam_forced_step
            tail.update(forced=d.ftab, max_len=max_len)
        step = functools.partial(launch, d.state, d.ldh, d.w_fc, d.b_fc, eos_id=self.eos, pad_id=self.pad, table=d.tbl4, base=d.zp4, add_out=d.add,
                                 score=score, fin=fin, ends=ends, hist_tok=hist_tok, hist_par=hist_par, B=B, K=K, V=d.V, H=d.H, **tail)
        rnn = d.rnn[0]                                        # the beam launch reorders the new state into half 0: no swap
        for i in range(1, max_len):
            rnn()
            step(step=i)
        ids = torch.empty((B, K, max_len), dtype=torch.long, device=dev)
        ends_out = torch.empty((B, K), dtype=torch.long, device=dev)
        scores = torch.empty((B, K), device=dev)
        ops.moses_beam_finalize(hist_tok, hist_par, ends, score, ids, ends_out, scores, self.bos, B, K, max_len)
        return ids, ends_out, scores

    @torch.no_grad()
    def score(self, x, z):
        """log p(x | z) per molecule: the teacher-forced decoder (no dropout) on the latents z [B, d_z], followed by mvae_ce_rows_fwd -- the
        raw summed log-probability of tokens 1 .. end of each sequence (the targets of the mean reconstruction loss).  x: a list of id
        tensors (bos first) or strings, in any order.  Returns a float32 [B] device tensor; no gradients."""
        seqs = self._seqs(x)
        B = len(seqs)
        if B < 1 or z.dim() != 2 or tuple(z.shape) != (B, self.d_z):
            raise ValueError(f"score: z must be [{B}, {self.d_z}], got {tuple(z.shape)}")
        dev = self.device
        _require_cuda(dev, "mosesvae.VAE.score")
        order, perm = length_order(seqs, dev)
        x_pad, len_t = self._batch([seqs[b].to(dev) for b in order])
        T, V = x_pad.shape[1], self.x_emb.num_embeddings
        # a workspace of its own: a pending forward_decoder's saved state (self._ws) stays intact
        ws = self.__dict__.setdefault("_score_ws", _Workspace())
        y_tb = _dec_forward(self, ws, self._pack(dev), x_pad, len_t, z.to(dev).float()[perm].contiguous(), None, heads=False)
        lp = torch.empty(B, device=dev)
        ops.ce_rows(y_tb, V, x_pad, self.pad, lp, B, T, V)
        out = torch.empty_like(lp)
        out[perm] = lp
        return out

    _IW_ROWS = 4096         # decoder rows per teacher-forced pass of iw_log_likelihood (bounds its workspace, not its result)

    @torch.no_grad()
    def iw_log_likelihood(self, x, n_samples=500, eps=None, seed=None):
        """Importance-weighted log-likelihood (Burda et al.; He et al. 2019 evaluate with K = 500): per molecule, the encoder's
        q(z | x) = N(mu, exp(logvar)) (eps = 0, as forward_encoder(x, eps=0)), K draws z_k = mu + exp(logvar / 2) * eps_k and
        log w_k = log p(x | z_k) + log N(z_k; 0, I) - log N(z_k; mu, sigma^2), log p(x | z_k) as `score` gives it.  Returns
        (log_px, elbo), fp32 [B] device tensors in input order: log_px = logsumexp_k log w_k - log K (-log_px is the NLL estimate) and
        elbo = mean_k log w_k over the same draws (log_px >= elbo).  x: id tensors (bos first) or strings, in any order.  eps [B, K, d_z]
        (input order) injects the noise; else it is drawn from self.noise_stream, or from a fresh stream of `seed`, molecule by molecule in
        the length-sorted order the decoder runs (a stable sort: molecules of equal length keep their input order).  So with drawn noise,
        a permutation of x permutes the result only when it keeps the relative order of molecules of equal length; two molecules of the
        same length that swap places also swap their draws.  No gradients, no dropout."""
        seqs = self._seqs(x)
        stream = ops.NoiseStream(seed) if seed is not None else self.noise_stream
        log_px, elbo, _, _ = self._iw(seqs, n_samples, eps, stream)
        return log_px, elbo

    def _iw(self, seqs, n_samples, eps, stream):
        """iw_log_likelihood on a list of id tensors; also returns the encoder's (mu, logvar) [B, d_z] in input order."""
        B, K, dz = len(seqs), int(n_samples), self.d_z
        if B < 1 or K < 1:
            raise ValueError(f"iw_log_likelihood: needs at least one molecule and n_samples >= 1, got {B} and {n_samples}")
        if eps is not None and tuple(eps.shape) != (B, K, dz):
            raise ValueError(f"iw_log_likelihood: eps must be [{B}, {K}, {dz}], got {tuple(eps.shape)}")
        dev = self.device
        _require_cuda(dev, "mosesvae.VAE.iw_log_likelihood")
        order, perm = length_order(seqs, dev)
        lens = [int(seqs[b].numel()) for b in order]
        x_pad, len_t = self._batch([seqs[b].to(dev) for b in order])
        V, f32 = self.x_emb.num_embeddings, torch.float32
        P = self._pack(dev)
        # workspaces of their own: a pending forward's saved state (self._ws) stays intact
        ws_e = self.__dict__.setdefault("_iw_enc_ws", _Workspace())
        mu, _, lv, _ = _enc_forward(self, ws_e, P, x_pad, len_t, torch.zeros(B, dz, device=dev))      # eps = 0: z = mu
        lv = lv.clone()
        if eps is None:
            seed_, off = stream.take(B * K * dz)
            eps_s = None
        else:
            seed_, off = 0, 0
            eps_s = eps.to(dev).float()[perm].reshape(B * K, dz).contiguous()
        lp, logw = torch.empty(B * K, device=dev), torch.empty(B * K, device=dev)
        ws = self.__dict__.setdefault("_iw_ws", _RowsWorkspace())      # one set of decoder buffers for passes of every (rows, T)
        R = self._IW_ROWS
        if K <= R:                                                       # whole molecules per pass
            chunks = [(b0, min(b0 + R // K, B), 0, K) for b0 in range(0, B, R // K)]
        else:                                                            # one molecule's draws over several passes
            chunks = [(b, b + 1, k0, min(k0 + R, K)) for b in range(B) for k0 in range(0, K, R)]
        for b0, b1, k0, k1 in chunks:
            nb, nk = b1 - b0, k1 - k0
            r0, rows, T = b0 * K + k0, nb * nk, lens[b0]
            z = ws.get("iw_z", (rows, dz), f32, dev)
            ops.gauss_iw_draw(mu[b0:b1], lv[b0:b1], z, logw[r0:r0 + rows], nb, nk, dz,
                              eps=None if eps_s is None else eps_s[r0:r0 + rows], seed=seed_, offset=off + r0 * dz)
            xc = x_pad[b0:b1, :T].repeat_interleave(nk, 0).contiguous()          # molecule-major: lengths stay descending
            y_tb = _dec_forward(self, ws, P, xc, len_t[b0:b1].repeat_interleave(nk, 0), z, None, heads=False)
            ops.ce_rows(y_tb, V, xc, self.pad, lp[r0:r0 + rows], rows, T, V)
        lme, mean = torch.empty(B, device=dev), torch.empty(B, device=dev)
        ops.group_logmeanexp(lp, lme, mean, B, K, b=logw)
        out = [torch.empty_like(t) for t in (lme, mean, mu, lv)]
        for o, t in zip(out, (lme, mean, mu, lv)):
            o[perm] = t
        return tuple(out)

    def _build_pack(self, dev):
        ws, dt, f32 = self._ws, self.compute_dtype, torch.float32
        V = self.x_emb.num_embeddings
        Vp = _pad(V, 4)
        P, pl = {}, ops.PackList()
        E = self.x_emb.weight
        P["E_p"] = ws.get("E_p", (V, Vp), f32, dev); P["ET_p"] = ws.get("ET_p", (V, Vp), f32, dev)
        pl.cast_transpose(E, V, V, dst=P["E_p"], dstT=P["ET_p"])
        for name, rnn in (("enc", self.encoder_rnn), ("dec", self.decoder_rnn)):
            H = rnn.hidden_size
            ldw, ldwT = H + _LDPAD, 4 * H + _LDPAD
            P[name] = dict(H=H, ldw=ldw, ldwT=ldwT, **_pack_rnn_stack(pl, ws, rnn, name + "_", dt, dev, ldw, ldwT))
            # layer-0 input weights: the embedding part becomes a table, the z part (decoder) a dense projection
            w0 = getattr(rnn, "weight_ih_l0")
            wx = ws.get(f"{name}_Wx_p", (3 * H, Vp), f32, dev); wxT = ws.get(f"{name}_WxT", (V, 3 * H), f32, dev)
            pl.cast_transpose(w0[:, :V], 3 * H, V, dst=wx, dstT=wxT)
            P[name]["Wx_p"], P[name]["WxT"] = wx, wxT
        dz = self.d_z
        Hd = P["dec"]["H"]
        w0 = self.decoder_rnn.weight_ih_l0
        P["Wz"] = ws.get("dec_Wz", (3 * Hd, dz), f32, dev); P["WzT"] = ws.get("dec_WzT", (dz, 3 * Hd), f32, dev)
        pl.cast_transpose(w0[:, V:], 3 * Hd, dz, dst=P["Wz"], dstT=P["WzT"])
        for n, seq in (("mu", self.q_mu), ("lv", self.q_logvar)):
            P[n + "_W0T"] = ws.get(n + "_W0T", (seq[0].in_features, seq[0].out_features), f32, dev)
            pl.cast_transpose(seq[0].weight, seq[0].out_features, seq[0].in_features, dstT=P[n + "_W0T"])
            P[n + "_W2T"] = ws.get(n + "_W2T", (seq[2].in_features, seq[2].out_features), f32, dev)
            pl.cast_transpose(seq[2].weight, seq[2].out_features, seq[2].in_features, dstT=P[n + "_W2T"])
        P["WlatT"] = ws.get("WlatT", (dz, Hd), f32, dev); pl.cast_transpose(self.decoder_lat.weight, Hd, dz, dstT=P["WlatT"])
        Vp8 = _pad(V, 8)
        P["Wfc"] = ws.get("Wfc", (V, Hd + _LDPAD), dt, dev); P["WfcT"] = ws.get("WfcT", (Hd, _dyk(V) if dt == torch.bfloat16 else Vp8), dt, dev)
        pl.cast_transpose(self.decoder_fc.weight, V, Hd, dst=P["Wfc"], dstT=P["WfcT"])
        self._set_pack(P, pl)


# ------------------------------------------------------------------------------------------------------------------------------------
# The two halves of the step (mosesvae.py:142-164 encoder, :166-199 decoder) as helpers over a workspace.  Three autograd Functions are built
# from them: _MosesFn (the fused `forward`, mosesvae.py:126-140: both halves in one node, decoder parameter gradients on a side stream beside
# the encoder's backward), _MosesEncFn (`forward_encoder`: the encoder half alone) and _MosesDecFn (`forward_decoder(x, z)`: the decoder half
# on a latent the caller supplies, with a gradient w.r.t. that latent).  The halves use disjoint buffer names and keep a generation count
# each (`_SavedState._next_saved_ws(half)`), so `forward_encoder` followed by `forward_decoder` (the reference's composition) overwrites nothing.
class SmilesView(SmilesReaders):
    """``SmilesReaders`` under ANOTHER vocabulary than the model's: what ``moses_generate(selfies=)`` runs on the SMILES rows a SELFIES
    model's samples decode to.  It supplies what the readers ask of ``self``: the vocabulary and its ids, the model's device, the
    per-vocabulary tables (cached here) and the row intake."""

    def __init__(self, model, vocab):
        self.model, self.vocabulary = model, vocab
        self.bos, self.eos, self.pad = vocab.bos, vocab.eos, vocab.pad
        self._tables = {}

    device = property(lambda self: self.model.device)

    def _vocab_table(self, key, build, dev):
        if (key, None) not in self._tables:
            self._tables[key, None] = build(self.vocabulary)
        if dev is None:
            return self._tables[key, None]
        if (key, dev) not in self._tables:
            self._tables[key, dev] = self._tables[key, None].to(dev)
        return self._tables[key, dev]

    def _rows(self, x, who, dev=None):
        return token_rows(x, lambda s: self.vocabulary.string2ids(s, add_bos=True, add_eos=True), self.pad, who, dev)


def _opts(x_in, free_bits):
    """The collapse remedies of one forward as the autograd nodes carry them: None when both are off (the default path), else
    dict(x_in = the decoder's word-dropped input tokens | None, fb = None | dict(lam = free bits; the encoder half adds kl2, kl_dim))."""
    if x_in is None and not free_bits > 0.0:
        return None
    return dict(x_in=x_in, fb=dict(lam=free_bits) if free_bits > 0.0 else None)


def _enc_forward(mod, ws, P, x_pad, lengths, eps, fb=None):
    """fb (dict(lam), free bits on): the latent launch is mvae_moses_latent_fb_fwd; the returned kl is the objective, fb receives kl2
    (objective, KL) and kl_dim [d_z] (the workspace's copy: the backward's gate)."""
    dev, dt, f32 = x_pad.device, mod.compute_dtype, torch.float32
    B, T = x_pad.shape
    V, dz = mod.x_emb.num_embeddings, mod.d_z
    Vp = _pad(V, 4)
    W = lambda name, shape, d=f32: ws.get(name, shape, d, dev)
    # ---------------- encoder GRU (mosesvae.py:150-156): embedding folded into a [V, 4H] table
    pe = P["enc"]; Hq = pe["H"]
    tbl4 = W("enc_tbl4", (V, 4 * Hq)); ops.gemm_nt(P["E_p"], pe["Wx_p"], tbl4, V, 3 * Hq, Vp)      # slot 3 stays zero (ldc = 4H)
    # the table rows are added in the step epilogue (add_table / add_index): no gathered [T, B, 4H] copy
    ldh_e = Hq + _LDPAD
    hsx_e = [W("enc_hsx0", (T + 1, B, ldh_e), dt)]                 # slot 0 = initial state (zeros), slots 1.. = outputs
    gates_e = [W("enc_gates0", (T, B, 4 * Hq), dt)]
    hstate_e = [W("enc_hstate0", (2, B, Hq))]
    ops.rnn_fwd(L.CELL_GRU, dt, T, B, Hq, None, 0, pe["Wih"], [pe["ldw"]], pe["Whh"], [pe["ldw"]], pe["bias"],
                [hsx_e[0][1:]], ldh_e, None, gates_e, hstate_e, lengths=lengths, add_table=tbl4, add_index=x_pad, tag="moses_enc_fwd")
    h_last = hstate_e[0][(T - 1) & 1]                               # fp32 [B,Hq]: last valid state of every sequence
    # ---------------- heads + reparameterisation + KL (mosesvae.py:158-162)
    m1 = W("m1", (B, 256)); l1 = W("l1", (B, 256)); mu = W("mu", (B, dz)); lv = W("lv", (B, dz))
    ops.gemm_nt(h_last, mod.q_mu[0].weight, m1, B, 256, Hq, bias=mod.q_mu[0].bias, act=L.ACT_RELU)
    ops.gemm_nt(m1, mod.q_mu[2].weight, mu, B, dz, 256, bias=mod.q_mu[2].bias)
    ops.gemm_nt(h_last, mod.q_logvar[0].weight, l1, B, 256, Hq, bias=mod.q_logvar[0].bias, act=L.ACT_RELU)
    ops.gemm_nt(l1, mod.q_logvar[2].weight, lv, B, dz, 256, bias=mod.q_logvar[2].bias)
    z = torch.empty(B, dz, device=dev); kl = torch.empty(1 if fb is None else 2, device=dev)
    if fb is not None:
        fb["kl2"], fb["kl_dim"] = kl, W("kl_dim", (dz,))
        latent = lambda e, **k: ops.moses_latent_fb_fwd(mu, lv, e, z, kl, fb["kl_dim"], B, dz, fb["lam"], **k)
    else:
        latent = lambda e, **k: ops.moses_latent_fwd(mu, lv, e, z, kl, B, dz, **k)
    if eps is None:
        seed, off = mod.noise_stream.take(B * dz)
        eps = W("eps", (B, dz))
        latent(None, seed=seed, offset=off, eps_out=eps)
    else:
        latent(eps)
    return z, kl, lv, eps


def _dec_forward(mod, ws, P, x_pad, lengths, z, drop, heads=True, x_in=None):
    """heads=False: return the time-major logits y_tb [T*B, V] alone (no `y` permute, no mean cross-entropy; VAE.score).
    x_in (word dropout): the tokens the GRU READS; the cross-entropy targets stay x_pad."""
    dev, dt, f32 = x_pad.device, mod.compute_dtype, torch.float32
    B, T = x_pad.shape
    V, dz = mod.x_emb.num_embeddings, mod.d_z
    Vp = _pad(V, 4)
    W = lambda name, shape, d=f32: ws.get(name, shape, d, dev)
    # ---------------- decoder (mosesvae.py:172-197)
    pd = P["dec"]; Hd = pd["H"]; NL = mod.decoder_rnn.num_layers
    W("z_saved", (B, dz)).copy_(z)                                  # the backward's operand (dW_z, decoder_lat): z is an output / input tensor we do not own
    h0 = W("h0", (B, Hd)); ops.gemm_nt(z, mod.decoder_lat.weight, h0, B, Hd, dz, bias=mod.decoder_lat.bias)
    tbl4d = W("dec_tbl4", (V, 4 * Hd)); ops.gemm_nt(P["E_p"], pd["Wx_p"], tbl4d, V, 3 * Hd, Vp)
    zp4 = W("zp4", (B, 4 * Hd)); ops.gemm_nt(z, P["Wz"], zp4, B, 3 * Hd, dz)
    ldh_d = Hd + _LDPAD
    hsx_d = [W(f"dec_hsx{l}", (T + 1, B, ldh_d), dt) for l in range(NL)]
    for l in range(NL):
        ops.cast_transpose(h0, B, Hd, dst=hsx_d[l][0])              # h_0 = decoder_lat(z) for every layer (mosesvae.py:185-186)
    gates_d = [W(f"dec_gates{l}", (T, B, 4 * Hd), dt) for l in range(NL)]
    hstate_d = [W(f"dec_hstate{l}", (2, B, Hd)) for l in range(NL)]
    hd = None
    if drop is not None:                                            # train mode: dropped copies of the outputs of layers 0 .. NL-2
        hd = [W(f"dec_hd{l}", (T, B, ldh_d), dt) for l in range(NL - 1)] + [None]
    # layer-0 input [emb(x_t), z] (mosesvae.py:176-188): z part = time-invariant addend zp4, token part = table row x[b, t]
    ops.rnn_fwd(L.CELL_GRU, dt, T, B, Hd, zp4, 0, pd["Wih"], [pd["ldw"]] * NL, pd["Whh"], [pd["ldw"]] * NL, pd["bias"],
                [h[1:] for h in hsx_d], ldh_d, None, gates_d, hstate_d, h0=[h[0] for h in hsx_d], ldh0=ldh_d, lengths=lengths,
                add_table=tbl4d, add_index=(x_pad if x_in is None else x_in),
                hdrop=hd, drop_mask=(None if drop is None or drop[2] is None else [drop[2][l] for l in range(NL - 1)]),
                drop_p=(drop[0] if drop else 0.0), drop_seed=(drop[1] if drop else 0), tag="moses_dec_fwd")
    TB = T * B
    y_tb = W("y_tb", (TB, V))
    ops.gemm_nt(hsx_d[-1][1:].reshape(TB, ldh_d), P["Wfc"], y_tb, TB, V, Hd, bias=mod.decoder_fc.bias)
    if not heads:
        return y_tb
    y = torch.empty(B, T, V, device=dev); ops.permute102(y_tb, y, T, B, V)
    loss2 = W("loss2", (2,)); ops.ce_loss_fwd(y_tb, V, x_pad, mod.pad, loss2, B, T, V)
    return loss2[0].clone(), y, loss2[1].clone()


def _lin_bwd(ws, grads, dev, B, tag, dy, x, WT, wname, bname, M_in, N_out, need_dx=True):
    """y = x W^T + b:  dW = dy^T x (exact-f32 TN kernel straight from the batch-major operands) with db = colsum(dy) as its virtual
    ones column, dx = dy W (via the packed transpose WT [in, out])."""
    ops.gemm_tn_f32_colsum(dy, x, grads[wname], grads[bname], N_out, M_in, B, lda=dy.stride(0), ldb=x.stride(0))
    if not need_dx:
        return None
    dx = ws.get(tag + "_dx", (B, M_in), torch.float32, dev)
    ops.gemm_nt(dy, WT, dx, B, M_in, N_out)
    return dx


def _onehot(mod, ws, x_pad, name="onehot_tb"):
    """bf16: the token scatter as a contraction, dtbl = onehot(x)^T . dG0 over the T*B rows (both halves' table gradients use the matrix;
    under word dropout the decoder half has a second one, of the tokens it read)."""
    dt = mod.compute_dtype
    if dt != torch.bfloat16:
        return None
    B, T = x_pad.shape
    V = mod.x_emb.num_embeddings
    oh = ws.get(name, (T * B + 8, _pad(V, 8)), dt, x_pad.device)[:T * B]
    ops.onehot_tb(x_pad, oh, B, T, V)
    return oh


def _dec_backward(mod, ws, P, grads, x_pad, lengths, drop, drecon, dy_ext, dz_ext, fork, onehot, x_in=None):
    """x_in (word dropout): the tokens the GRU read -- the table gradient is scattered by them (`onehot` is then THEIR matrix), the
    cross-entropy gradient still takes its targets from x_pad.
    Gradients of the decoder half: fills grads[decoder_*] and the decoder's share dE of the embedding gradient; returns (dz, finish) --
    dz [B, d_z] = gradient w.r.t. the latent (incl. dz_ext), finish() = the bias column sums + the join of the side stream, to be called
    once the caller has enqueued whatever it wants to run beside the side stream's weight-gradient GEMMs."""
    dev, dt, f32 = x_pad.device, mod.compute_dtype, torch.float32
    B, T = x_pad.shape
    V, dz = mod.x_emb.num_embeddings, mod.d_z
    Vp, Vp8, TB, Bp = _pad(V, 4), _pad(V, 8), T * B, _pad(B, 4)
    W = lambda name, shape, d=f32: ws.get(name, shape, d, dev)
    c = lambda t: t.contiguous().float() if t is not None else None
    g1 = lambda t: c(t).reshape(1) if t is not None else None
    pd = P["dec"]
    Hd, NL = pd["H"], mod.decoder_rnn.num_layers
    ldh_d = Hd + _LDPAD
    # ---------------- decoder_fc + cross-entropy
    y_tb, loss2 = W("y_tb", (TB, V)), W("loss2", (2,))
    fuse_dy = dt == torch.bfloat16 and (4 * Hd) % 64 == 0   # the top GRU cell contracts dl . W_fc itself (pad / finished positions: zero rows in dl)
    ldl = _dyk(V) if fuse_dy else Vp8
    dl = W("dl", (TB + 8, ldl), dt)[:TB]
    if drecon is None:
        drecon = torch.zeros((), device=dev)
    ops.ce_loss_bwd(y_tb, V, x_pad, mod.pad, loss2, g1(drecon), c(dy_ext), dl, B, T, V)
    hsx_d = [W(f"dec_hsx{l}", (T + 1, B, ldh_d), dt) for l in range(NL)]
    out_seq = hsx_d[-1][1:].reshape(TB, ldh_d)
    # Everything below that only produces PARAMETER gradients of the decoder (decoder_fc, the GRU stack's dW / db, the token table) is
    # throughput-bound and independent of dz, while what follows on the path to the encoder -- heads, the encoder GRU's reverse
    # pass: latency-bound, a fraction of the chip -- is not: the former runs on a side stream beside the latter (joined by finish()).
    side = mod._side_stream(dev) if fork else None

    def fc_grads():
        _kmajor_gemm(ws, "fc", dl, ldl, V, out_seq, ldh_d, Hd, TB, grads["decoder_fc.weight"], dev)
        dbp = W("dbfc_p", (Vp8,)); ops.colsum_t(dl, TB, Vp8, dbp, ldx=ldl); grads["decoder_fc.bias"].copy_(dbp[:V])

    if not fork:
        fc_grads()
    if fuse_dy and dy_ext is not None:
        # an external gradient w.r.t. the returned logits sits in dl at finished positions too (it counts for decoder_fc.bias, above); the
        # padded output carries no gradient back to h there (pad_packed_sequence, mosesvae.py:189), and the top cell contracts dl AS IS:
        # clear those rows first.  (The CE's own gradient is zero there already: the target is pad.)
        ops.mask_rows_tb(dl, T, B, lengths)
    dyd = None
    if not fuse_dy:
        dyd = W("dy_dec", (TB, Hd)); ops.gemm_nt(dl, P["WfcT"], dyd, TB, Hd, Vp8)
    # ---------------- decoder GRU stack, reverse wavefront (+ gradient w.r.t. h_0 of every layer)
    ldg_d = 4 * Hd + _LDPAD
    gates_d = [W(f"dec_gates{l}", (T, B, 4 * Hd), dt) for l in range(NL)]
    dG_d = [W(f"dec_dG{l}", (T, B, ldg_d), dt) for l in range(NL)]
    dstate_d = [W(f"dec_dstate{l}", (2, B, Hd)) for l in range(NL)]
    dh0 = [W(f"dec_dh0_{l}", (B, Hd)) for l in range(NL)]
    ops.rnn_bwd(L.CELL_GRU, dt, T, B, Hd, pd["WhhT"], [pd["ldwT"]] * NL, pd["WihT"], [pd["ldwT"]] * NL, dyd, Hd,
                [h[1:] for h in hsx_d], ldh_d, None, gates_d, dG_d, dstate_d, ldg=ldg_d, h0=[h[0] for h in hsx_d], ldh0=ldh_d,
                lengths=lengths, dh0=dh0,
                drop_mask=(None if drop is None or drop[2] is None else [drop[2][l] for l in range(NL - 1)]),
                drop_p=(drop[0] if drop else 0.0), drop_seed=(drop[1] if drop else 0), tag="moses_dec_bwd",
                dy_a=(dl if fuse_dy else None), dy_w=(P["WfcT"] if fuse_dy else None), dy_k=(_dyk(V) if fuse_dy else 0))
    hd = [W(f"dec_hd{l}", (T, B, ldh_d), dt) for l in range(NL - 1)] if drop is not None else None
    dE = grads["_dE_dec"]

    def dec_bias_grads():
        # column sums of dG (bandwidth-bound passes over [T*B, 4H]): on the MAIN stream behind the encoder's backward, beside the side
        # stream's compute-bound weight-gradient GEMMs -- the side stream is the longer of the two chains since the encoder's backward is one launch
        s4 = W("dec_s4", (4 * Hd,))
        for l in range(NL):
            _gru_param_grads(ws, "", grads, "decoder_rnn", l, dG_d[l].view(TB, ldg_d), ldg_d, None, None, ldh_d, Hd, TB, dev, s4=s4)

    def dec_weight_grads():
        # the 3 x (dW_hh[r, z], dW_hh[n], dW_ih) contractions of the stack, one split-K TN GEMM each (one grouped launch of full-K 256 x 256
        # tiles measured slower in round 5: 5.46 vs 5.18 ms per step at B = 1024)
        for l in range(NL):
            hprev = hsx_d[l][:T].reshape(TB, ldh_d)                  # h_{t-1} for every t (slot 0 = h_0)
            xin = None                                                # the layer's input: the output of layer l-1 (after its dropout in train mode)
            if l > 0:
                xin = hd[l - 1].view(TB, ldh_d) if hd is not None else hsx_d[l - 1][1:].reshape(TB, ldh_d)
            _gru_param_grads(ws, "", grads, "decoder_rnn", l, dG_d[l].view(TB, ldg_d), ldg_d, hprev, xin, ldh_d, Hd, TB, dev)
        # layer-0 input = [emb(x_t), z]: table gradient for the embedding part (the z part is on the path to the encoder: main stream)
        dtbl3 = W("dec_dtbl3", (V, 3 * Hd))
        if onehot is not None:
            ops.gemm_tn(onehot, dG_d[0].view(TB, ldg_d), dtbl3, V, 3 * Hd, TB, lda=Vp8, ldb=ldg_d)
        else:
            dtbl4 = W("dec_dtbl4", (V, 4 * Hd)); ops.scatter_rows_tb(x_pad if x_in is None else x_in, dG_d[0], dtbl4, B, T, V, 4 * Hd, ldd=ldg_d)
            dtbl3.copy_(dtbl4[:, :3 * Hd])
        ops.gemm_nt(dtbl3, pd["WxT"], dE, V, V, 3 * Hd)
        dtblT = W("dec_dtblT", (3 * Hd, Vp)); ops.cast_transpose(dtbl3, V, 3 * Hd, dstT=dtblT)
        dwx = W("dec_dwx", (3 * Hd, V)); ops.gemm_nt(dtblT, P["ET_p"], dwx, 3 * Hd, V, Vp)
        grads["decoder_rnn.weight_ih_l0"][:, :V].copy_(dwx)

    side_done = None
    if fork:
        ev = torch.cuda.Event(); ev.record()
        side.wait_event(ev)
        for t in grads["_flat"]:
            t.record_stream(side)
        with torch.cuda.stream(side):
            fc_grads()
            dec_weight_grads()
            side_done = torch.cuda.Event(); side_done.record()
    else:
        dec_weight_grads()
    dzp4 = W("dzp4", (B, ldg_d)); ops.timesum(dG_d[0], T, B, ldg_d, dzp4)
    dzp3 = W("dzp3", (B, 3 * Hd)); dzp3.copy_(dzp4[:, :3 * Hd])
    z = W("z_saved", (B, dz))
    dzp3T, zT = W("dzp3T", (3 * Hd, Bp)), W("zT", (dz, Bp))
    ops.cast_transpose(dzp3, B, 3 * Hd, dstT=dzp3T); ops.cast_transpose(z, B, dz, dstT=zT)
    dwz = W("dec_dwz", (3 * Hd, dz)); ops.gemm_nt(dzp3T, zT, dwz, 3 * Hd, dz, Bp)
    grads["decoder_rnn.weight_ih_l0"][:, V:].copy_(dwz)          # (the token columns [:, :V] are written by dec_weight_grads)
    dz_tot = W("dz_tot", (B, dz)); ops.gemm_nt(dzp3, P["WzT"], dz_tot, B, dz, 3 * Hd)
    # h_0 = decoder_lat(z), shared by the layers
    dh0s = dh0[0]
    for l in range(1, NL):
        dh0s.add_(dh0[l])
    dzl = _lin_bwd(ws, grads, dev, B, "lat", dh0s, z, P["WlatT"], "decoder_lat.weight", "decoder_lat.bias", dz, Hd)
    dz_tot.add_(dzl)
    if dz_ext is not None:
        dz_tot.add_(c(dz_ext))

    def finish():
        dec_bias_grads()
        if side_done is not None:
            torch.cuda.current_stream().wait_event(side_done)        # the decoder's parameter gradients (and dE) from the side stream

    return dz_tot, finish


def _enc_backward(mod, ws, P, grads, x_pad, lengths, eps, dz_tot, dkl, dlv_ext, onehot, fb=None):
    """Gradients of the encoder half from dz_tot [B, d_z] (None: no gradient through z), the KL weight and an external gradient w.r.t. logvar:
    fills grads[encoder_rnn.*, q_mu.*, q_logvar.*] and the encoder's share dE2 of the embedding gradient.  fb: the forward's free-bits record."""
    dev, dt, f32 = x_pad.device, mod.compute_dtype, torch.float32
    B, T = x_pad.shape
    V, dz = mod.x_emb.num_embeddings, mod.d_z
    Vp, Vp8, TB = _pad(V, 4), _pad(V, 8), T * B
    W = lambda name, shape, d=f32: ws.get(name, shape, d, dev)
    c = lambda t: t.contiguous().float() if t is not None else None
    g1 = lambda t: c(t).reshape(1) if t is not None else None
    pe = P["enc"]
    Hq = pe["H"]
    ldh_e = Hq + _LDPAD
    lin_bwd = lambda *a, **k: _lin_bwd(ws, grads, dev, B, *a, **k)
    # ---------------- reparameterisation + KL, heads
    mu, lv = W("mu", (B, dz)), W("lv", (B, dz))
    dmu, dlv = W("dmu", (B, dz)), W("dlv", (B, dz))
    if dz_tot is None:
        dz_tot = W("dz_zero", (B, dz))                                # allocated zero, never written
    if fb is not None:
        ops.moses_latent_fb_bwd(mu, lv, eps, dz_tot, g1(dkl), c(dlv_ext), W("kl_dim", (dz,)), fb["lam"], dmu, dlv, B, dz)
    else:
        ops.moses_latent_bwd(mu, lv, eps, dz_tot, g1(dkl), c(dlv_ext), dmu, dlv, B, dz)
    m1, l1 = W("m1", (B, 256)), W("l1", (B, 256))
    h_last = W("enc_hstate0", (2, B, Hq))[(T - 1) & 1]
    dm1 = lin_bwd("mu2", dmu, m1, P["mu_W2T"], "q_mu.2.weight", "q_mu.2.bias", 256, dz); ops.relu_bwd(dm1, m1)
    dhq = lin_bwd("mu0", dm1, h_last, P["mu_W0T"], "q_mu.0.weight", "q_mu.0.bias", Hq, 256)
    dhq_tot = W("dhq_tot", (B, Hq)); dhq_tot.copy_(dhq)
    dl1 = lin_bwd("lv2", dlv, l1, P["lv_W2T"], "q_logvar.2.weight", "q_logvar.2.bias", 256, dz); ops.relu_bwd(dl1, l1)
    dhq2 = lin_bwd("lv0", dl1, h_last, P["lv_W0T"], "q_logvar.0.weight", "q_logvar.0.bias", Hq, 256)
    dhq_tot.add_(dhq2)
    # ---------------- encoder GRU: only the final state receives gradient; masked steps pass it back to each sequence's last step
    ldg_e = 4 * Hq + _LDPAD
    hsx_e = [W("enc_hsx0", (T + 1, B, ldh_e), dt)]
    gates_e = [W("enc_gates0", (T, B, 4 * Hq), dt)]
    dG_e = [W("enc_dG0", (T, B, ldg_e), dt)]
    dstate_e = [W("enc_dstate0", (2, B, Hq))]
    ops.rnn_bwd(L.CELL_GRU, dt, T, B, Hq, pe["WhhT"], [pe["ldwT"]], pe["WihT"], [pe["ldwT"]], None, 0,
                [hsx_e[0][1:]], ldh_e, None, gates_e, dG_e, dstate_e, ldg=ldg_e, h0=[hsx_e[0][0]], ldh0=ldh_e,
                lengths=lengths, dh_last=[dhq_tot], tag="moses_enc_bwd")
    a = dG_e[0].view(TB, ldg_e)
    # "e_": the decoder's weight gradients may still run on the side stream in this workspace (_MosesFn, saved_state_depth 1)
    _gru_param_grads(ws, "e_", grads, "encoder_rnn", 0, a, ldg_e, hsx_e[0][:T].reshape(TB, ldh_e), None, ldh_e, Hq, TB, dev, s4=W("enc_s4", (4 * Hq,)))
    etbl3 = W("enc_dtbl3", (V, 3 * Hq))
    if onehot is not None:
        ops.gemm_tn(onehot, a, etbl3, V, 3 * Hq, TB, lda=Vp8, ldb=ldg_e)
    else:
        etbl4 = W("enc_dtbl4", (V, 4 * Hq)); ops.scatter_rows_tb(x_pad, dG_e[0], etbl4, B, T, V, 4 * Hq, ldd=ldg_e)
        etbl3.copy_(etbl4[:, :3 * Hq])
    ops.gemm_nt(etbl3, pe["WxT"], grads["_dE_enc"], V, V, 3 * Hq)
    etblT = W("enc_dtblT", (3 * Hq, Vp)); ops.cast_transpose(etbl3, V, 3 * Hq, dstT=etblT)
    ops.gemm_nt(etblT, P["ET_p"], grads["encoder_rnn.weight_ih_l0"], 3 * Hq, V, Vp)


def _moses_grad_views(mod, ws, names, params, dev):
    """_grad_views plus the two halves' scratch shares of the embedding gradient."""
    grads = _grad_views(names, params, dev)
    V = mod.x_emb.num_embeddings
    grads["_dE_dec"] = ws.get("dE", (V, V), torch.float32, dev)
    grads["_dE_enc"] = ws.get("dE2", (V, V), torch.float32, dev)
    return grads


class _MosesFn(torch.autograd.Function):
    """mosesvae.VAE.forward (mosesvae.py:126-140): both halves in ONE autograd node."""

    @staticmethod
    @ops.traced("moses_step_fwd")
    def forward(ctx, mod, x_pad, lengths, eps, drop, opt, *params):
        dev = x_pad.device
        _require_cuda(dev, "mosesvae.VAE")
        P = mod._pack(dev)
        slot, ws, gen = mod._next_saved_ws("enc")
        dslot, dws, dgen = mod._next_saved_ws("dec")
        x_in, fb = (opt["x_in"], opt["fb"]) if opt else (None, None)
        z, kl, lv, eps = _enc_forward(mod, ws, P, x_pad, lengths, eps, fb)
        recon, y, ntok = _dec_forward(mod, dws, P, x_pad, lengths, z, drop, x_in=x_in)
        ctx.mod, ctx.x_pad, ctx.lengths, ctx.eps, ctx.drop, ctx.x_in, ctx.fb = mod, x_pad, lengths, eps, drop, x_in, fb
        ctx.slot, ctx.gen, ctx.dslot, ctx.dgen = slot, gen, dslot, dgen
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(ntok)
        return kl[0].clone(), recon, z, lv.clone(), y, ntok

    @staticmethod
    @ops.traced("moses_step_bwd")
    def backward(ctx, dkl, drecon, dz_ext, dlv_ext, dy_ext, _dntok=None):
        mod, x_pad, lengths, eps, drop = ctx.mod, ctx.x_pad, ctx.lengths, ctx.eps, ctx.drop
        ws = mod._saved_ws(ctx.slot, ctx.gen, "mosesvae.VAE", "enc")
        dws = mod._saved_ws(ctx.dslot, ctx.dgen, "mosesvae.VAE", "dec")
        dev = x_pad.device
        P = mod._packed
        params = mod._plist()
        names = [n for n, _ in mod.named_parameters()]
        grads = _moses_grad_views(mod, ws, names, params, dev)
        onehot = _onehot(mod, ws, x_pad)
        x_in = ctx.x_in
        onehot_d = onehot if x_in is None else _onehot(mod, dws, x_in, "onehot_tb_in")     # the decoder scatters by the tokens it read
        dz_tot, finish = _dec_backward(mod, dws, P, grads, x_pad, lengths, drop, drecon, dy_ext, dz_ext, dy_ext is None, onehot_d, x_in)
        _enc_backward(mod, ws, P, grads, x_pad, lengths, eps, dz_tot, dkl, dlv_ext, onehot, ctx.fb)
        finish()
        ge = grads["x_emb.weight"]; torch.add(grads["_dE_dec"], grads["_dE_enc"], out=ge)
        ge[mod.pad].zero_()                                           # nn.Embedding(padding_idx=pad): no gradient to the pad row
        return (None, None, None, None, None, None) + tuple(grads[n] for n in names)


class _MosesEncFn(torch.autograd.Function):
    """mosesvae.VAE.forward_encoder (mosesvae.py:142-164): the encoder half ALONE -- no decoder kernel is launched."""

    @staticmethod
    @ops.traced("moses_encoder_fwd")
    def forward(ctx, mod, x_pad, lengths, eps, opt, *params):
        dev = x_pad.device
        _require_cuda(dev, "mosesvae.VAE.forward_encoder")
        P = mod._pack(dev)
        slot, ws, gen = mod._next_saved_ws("enc")
        fb = opt["fb"] if opt else None
        z, kl, lv, eps = _enc_forward(mod, ws, P, x_pad, lengths, eps, fb)
        ctx.mod, ctx.slot, ctx.gen, ctx.x_pad, ctx.lengths, ctx.eps, ctx.fb = mod, slot, gen, x_pad, lengths, eps, fb
        ctx.set_materialize_grads(False)
        return z, kl[0].clone(), lv.clone()

    @staticmethod
    @ops.traced("moses_encoder_bwd")
    def backward(ctx, dz_ext, dkl, dlv_ext):
        mod, x_pad, lengths, eps = ctx.mod, ctx.x_pad, ctx.lengths, ctx.eps
        ws = mod._saved_ws(ctx.slot, ctx.gen, "mosesvae.VAE.forward_encoder", "enc")
        dev = x_pad.device
        names, params = mod._half_params("enc")
        grads = _moses_grad_views(mod, ws, names, params, dev)
        onehot = _onehot(mod, ws, x_pad)
        dz = dz_ext.contiguous().float() if dz_ext is not None else None
        _enc_backward(mod, ws, mod._packed, grads, x_pad, lengths, eps, dz, dkl, dlv_ext, onehot, ctx.fb)
        ge = grads["x_emb.weight"]; ge.copy_(grads["_dE_enc"])
        ge[mod.pad].zero_()
        return (None, None, None, None, None) + tuple(grads[n] for n in names)


class _MosesDecFn(torch.autograd.Function):
    """mosesvae.VAE.forward_decoder (mosesvae.py:166-199): teacher-forced decoder on a latent the caller supplies; differentiable in z."""

    @staticmethod
    @ops.traced("moses_decoder_fwd")
    def forward(ctx, mod, x_pad, lengths, z, drop, opt, *params):
        dev = x_pad.device
        _require_cuda(dev, "mosesvae.VAE.forward_decoder")
        P = mod._pack(dev)
        dslot, dws, dgen = mod._next_saved_ws("dec")
        x_in = opt["x_in"] if opt else None
        recon, y, ntok = _dec_forward(mod, dws, P, x_pad, lengths, z.contiguous().float(), drop, x_in=x_in)
        ctx.mod, ctx.x_pad, ctx.lengths, ctx.drop, ctx.x_in = mod, x_pad, lengths, drop, x_in
        ctx.dslot, ctx.dgen = dslot, dgen
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(ntok)
        return recon, y, ntok

    @staticmethod
    @ops.traced("moses_decoder_bwd")
    def backward(ctx, drecon, dy_ext, _dntok=None):
        mod, x_pad, lengths, drop = ctx.mod, ctx.x_pad, ctx.lengths, ctx.drop
        ws = mod._saved_ws(ctx.dslot, ctx.dgen, "mosesvae.VAE.forward_decoder", "dec")
        dev = x_pad.device
        names, params = mod._half_params("dec")
        grads = _moses_grad_views(mod, ws, names, params, dev)
        x_in = ctx.x_in
        onehot = _onehot(mod, ws, x_pad if x_in is None else x_in)
        dz_tot, finish = _dec_backward(mod, ws, mod._packed, grads, x_pad, lengths, drop, drecon, dy_ext, None, dy_ext is None, onehot, x_in)
        finish()
        ge = grads["x_emb.weight"]; ge.copy_(grads["_dE_dec"])
        ge[mod.pad].zero_()
        dz = dz_tot.clone() if ctx.needs_input_grad[3] else None
        return (None, None, None, dz, None, None) + tuple(grads[n] for n in names)
