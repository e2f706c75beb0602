"""Writes the rows of the rewrite tests (the mutation corpus, rewrite_ref.HAND_ROWS, the refusal rows of tests/test_smiles_rewrite_host.py)
and the vocabulary's tables in the format tests/sanitize/rewrite_host_main.cpp reads.  Not a pytest file.

    python tests/sanitize/rewrite_host_dump.py rows.bin
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from molecular_vae_amd import vocab as VC   # noqa: E402
import chem_ref as CR   # noqa: E402
import rewrite_ref as RR   # noqa: E402
import test_smiles_rewrite_host as TH   # noqa: E402

v = CR.vocabulary()
rows = CR.mutation_corpus() + RR.HAND_ROWS + [TH.LADDER, TH.COMB, "C" * 128, "C[C@H](N)O", "F/C=C/F"] + RR.fragment_corpus(500, seed=3)
x = CR.token_rows(rows, v, 131)
x[5, 4] = -1                                                       # ids outside the vocabulary, and a row without <eos>
x[6, 2] = len(v)
x[7][x[7] == v.eos] = v.pad
draw = (np.arange(len(rows), dtype=np.uint64) * 2654435761 + 12345).astype(np.uint32)
with open(sys.argv[1], "wb") as f:
    np.array([x.shape[0], x.shape[1], len(v), v.bos, v.eos, v.pad, 20171031, 0], np.int32).tofile(f)
    x.astype(np.int64).tofile(f)
    for t in (VC.smiles_token_table(v), VC.smiles_chem_table(v), VC.smiles_emit_table(v)):
        t.numpy().astype(np.int32).tofile(f)
    draw.tofile(f)
print(len(rows), "rows of", x.shape[1], "columns")
