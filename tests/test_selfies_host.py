"""SELFIES on the host (no GPU): the mvae_selfies_decode_host / mvae_selfies_encode_host entries -- the same source as the kernels,
compiled for the CPU -- against a hand table, against selfies_ref (a pure-Python statement of the rules of include/mvae.h, "SELFIES"),
and through the round trip that needs no oracle; vocab.SelfiesVocab and its two tables.  Graphs are compared as token rows of
ops.smiles_canon_host.  Agreement with the selfies package is neither tested nor claimed."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from molecular_vae_amd import _lib as L, vocab as VC, ops
import chem_ref as CR
import kekule_ref as KR
import rewrite_ref as RR
import scaffold_ref as SR
import selfies_ref as SF
import test_smiles_aromatize_host as TA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 5
_CACHE = {}


def svocab():
    if "sv" not in _CACHE:
        _CACHE["sv"] = VC.SelfiesVocab.default()
    return _CACHE["sv"]


def smiles_tables(v):
    return VC.smiles_token_table(v), VC.smiles_chem_table(v), VC.smiles_emit_table(v)


def selfies_rows(texts, sv, T=None):
    """int64 [B, T] rows of SELFIES texts (<bos>, ids, <eos>, <pad>); a text may hold specials such as <pad>."""
    ids = [[sv.bos] + [sv.c2i[s] if s in sv.c2i else sv.symbol2id(s) for s in SF.split(t)] + [sv.eos] for t in texts]
    T = max(map(len, ids)) if T is None else T
    x = np.full((len(ids), T), sv.pad, np.int64)
    for b, row in enumerate(ids):
        x[b, :len(row)] = row
    return x


def decode_host(x, sv, v=None, **kw):
    v = CR.vocabulary() if v is None else v
    out = ops.selfies_decode_host(torch.as_tensor(x), VC.selfies_info_table(sv), VC.smiles_emit_table(v), v.bos, v.eos, v.pad, **kw)
    return tuple(t.numpy() for t in out)


def encode_host(strings, sv, v=None, T=None, **kw):
    v = CR.vocabulary() if v is None else v
    x = torch.from_numpy(CR.token_rows(strings, v, T))
    out = ops.selfies_encode_host(x, *smiles_tables(v), v.eos, VC.selfies_emit_table(sv), sv.bos, sv.eos, sv.pad, **kw)
    return tuple(t.numpy() for t in out)


def canon_host(strings, v=None):
    v = CR.vocabulary() if v is None else v
    out, out_len, status, _, _ = ops.smiles_canon_host(torch.from_numpy(CR.token_rows(strings, v)), *smiles_tables(v), v.bos, v.eos, v.pad,
                                                       info=False, rank=False)
    return out.numpy(), out_len.numpy(), status.numpy()


def aromatize_host(x, v=None):
    v = CR.vocabulary() if v is None else v
    out, out_len, status, _, _ = ops.smiles_aromatize_host(torch.as_tensor(x), *smiles_tables(v), v.bos, v.eos, v.pad, info=False, arom=False)
    return out.numpy(), out_len.numpy(), status.numpy()


def same_row(a, na, b, nb):
    return na == nb and np.array_equal(a[:na], b[:nb])


def smiles_text(row, n, v):
    return "".join(v.i2c[int(i)] for i in row[1:n - 1])


def mates(strings, v=None):
    """Per string the mates of the atoms of N as the kekule host entry gives them ({} without aromatic atoms, None where it does not
    kekulise or the walk refuses the row): the matching the definition names."""
    v = CR.vocabulary() if v is None else v
    ti, ci, _ = smiles_tables(v)
    status, _, mate = ops.smiles_kekule_host(torch.from_numpy(CR.token_rows(strings, v)), ti, ci, v.eos)
    return [None if int(st) != 0 else {a: int(m) for a, m in enumerate(row.tolist()) if m != 255} for st, row in zip(status, mate)]


def multiple_ring_bond(atoms):
    """whether some bond that lies on a cycle (a non-bridge edge: scaffold_ref's low-link search) has order >= 2"""
    return any(atoms[a]["nb"][b] >= 2 for a, b in map(tuple, SR.ring_bonds(atoms)))


def test_entries_are_declared_bound_and_built():
    text = open(os.path.join(ROOT, "include", "mvae.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = L.load()
    for name in [f"mvae_selfies_{d}_{k}" for d in ("decode", "encode") for k in ("rows", "corpus", "host")]:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert int(re.search(r"#define\s+MVAE_SELFIES_CAPACITY\s+(\d+)", header).group(1)) == ops.SELFIES_STATUS_CAPACITY == 18
    assert len(ops.SELFIES_STATUS_NAMES) == 19 and ops.SELFIES_STATUS_NAMES[18] == "selfies_capacity"
    assert int(re.search(r"#define\s+MVAE_SELFIES_EMIT\s+(\d+)", header).group(1)) == ops.SELFIES_EMIT == VC.SELFIES_EMIT_WORDS == 529
    assert int(re.search(r"#define\s+MVAE_SELFIES_COUNTS\s+(\d+)", header).group(1)) == ops.SELFIES_COUNTS == 32
    assert "agreement\n *   with the package is neither tested nor claimed" in text
    build = open(os.path.join(ROOT, "molecular-vae_amd", "csrc", "build.sh")).read()
    assert build.count(" selfies ") == 2 and "build/selfies.o" in build and "build/tune/selfies.o" in build
    # the matching, the adjacency, the ranks and the writer are shared, not copied
    csrc = os.path.join(ROOT, "molecular-vae_amd", "csrc")
    src = open(os.path.join(csrc, "selfies.hip")).read() + open(os.path.join(csrc, "selfies.hpp")).read()
    assert all(f'#include "{h}"' in src for h in ("kekule.hpp", "smiles_canon.hpp", "smiles_writer.hpp"))
    assert "common_base" not in src and "EM_LPAR" not in src and "__syncthreads" not in src


def test_new_kernels_use_no_scratch(tmp_path):
    """The compiler's resource remarks for the four kernels of selfies.hip: scratch 0, no spills, the LDS per block include/mvae.h states."""
    csrc = os.path.join(ROOT, "molecular-vae_amd", "csrc")
    usage = os.path.join(csrc, "build", "selfies.usage.txt")
    sources = ("selfies.hip", "selfies.hpp", "kekule.hpp", "smiles_canon.hpp", "smiles_writer.hpp", "smiles_rounds.hpp", "smiles_graph.hpp",
               "smiles_syntax.hpp", "common.hpp", "../../include/mvae.h")
    if os.path.exists(usage) and os.path.getmtime(usage) >= max(os.path.getmtime(os.path.join(csrc, f)) for f in sources):
        text = open(usage, errors="replace").read()
    else:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        run = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                              "-c", os.path.join(csrc, "selfies.hip"), "-o", str(tmp_path / "selfies.dev.o")],
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert run.returncode == 0, run.stderr[-2000:]
        text = run.stderr
    names = re.findall(r"Function Name: (\S+)", text)
    assert len(names) == 4 and all(any(k in n for n in names) for k in ("selfies_decode_rows_kernel", "selfies_decode_corpus_kernel",
                                                                        "selfies_encode_rows_kernel", "selfies_encode_corpus_kernel")), names
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text) == ["0"] * 4
    assert re.findall(r"VGPRs Spill: (\d+)", text) == ["0"] * 4 and re.findall(r"SGPRs Spill: (\d+)", text) == ["0"] * 4
    header = open(os.path.join(ROOT, "include", "mvae.h")).read()
    stated = int(re.search(r"#define\s+MVAE_SELFIES_LDS_BYTES\s+(\d+)", header).group(1))
    assert list(map(int, re.findall(r"LDS Size \[bytes/block\]: (\d+)", text))) == [stated] * 4 and stated <= 81920
    assert all(int(n) <= 128 for n in re.findall(r" VGPRs: (\d+)", text))


# (SELFIES, the SMILES it denotes or None for status 1, info[3] for status 1)
HAND = [
    ("[C][C][O]", "CCO"),
    ("[C][=C][C][=C][C][=C][Ring1][=Branch1]", "C1=CC=CC=C1"),
    ("[C][C][Branch1][C][F][C]", "CC(F)C"),
    ("[C][F][C]", "CF"),
    ("[C][#O]", "C=O"),
    ("[O][=O][=O]", "O=O"),
    ("[C][Ring1][C]", "C"),
    ("[F][Branch1][C][C]", "FCC"),
    ("[C][C][Ring1][C]", "C=C"),
    ("[C][C][Ring1][C][Ring1][C][Ring1][C]", "C#C"),
    ("[C][C][C][=Ring1][Ring1]", "C1=CC1"),
    ("[C][NH1][C]", "C[NH]C"),
    ("[C][N+1][=Branch1][C][=O][O-1]", "C[N+](=O)[O-]"),
    ("[NH1][C]", "[NH]C"),
    ("[C][C][Branch1][Ring1][C][C][C][O]", "CC(CC)CO"),
    ("[C][nop][C][=Branch1]", "CC"),
    ("[C]<pad>[C]", None, 2),
    ("<pad>", None, 1),
    ("[C]<unk>", None, 2),
    ("", None, 1),
    ("[nop][Ring1][Branch1]", None, 4),
]


def test_hand_table():
    """Derived by hand from the definition (s = the bonds the previous atom can still make):
      [C][C][O]                  C s=4; C o=1 s=3; O o=1 s=1                                                       CCO
      [C][=C][C][=C][C][=C][Ring1][=Branch1]   the chain C=C-C=C-C=C, atom 5 has s=2; Ring1 reads Q = index([=Branch1]) = 4, so
                                 l = 5 - 5 = 0, o = 1: the ring bond 0-5                                           benzene, Kekule
      [C][C][Branch1][C][F][C]   at atom 1 s=3: b = min(2, 1) = 1, Q = index([C]) = 0, so the branch is the one symbol [F]; the chain
                                 resumes at atom 1 with s=2 and takes [C]                                          CC(F)C
      [C][F][C]                  F: o=1, s = 1 - 1 = 0: the chain ends, the last [C] is consumed without effect    CF
      [C][#O]                    o = min(3, 4, cap(O) = 2) = 2                                                     C=O
      [O][=O][=O]                O s=2; =O o=2, s=0: the chain ends                                                O=O
      [C][Ring1][C]              Ring1 at s=4: Q = index([C]) = 0 is CONSUMED, l = max(0, 0 - 1) = 0 = r: skipped when applied       C
      [F][Branch1][C][C]         F s=1: Branch1 at s <= 1 is skipped and its index symbol [C] is read as an atom: F-C, then -C       FCC
      [C][C][Ring1][C]           Ring1 at atom 1: Q=0, l=0, r=1, which the tree bond joins already: it is raised by min(1, 3-1)      C=C
      ... [Ring1][C][Ring1][C]   twice more: order 3, then min(1, 3-3) = 0                                         C#C
      [C][C][C][=Ring1][Ring1]   at atom 2 s=3: o = min(2, 3) = 2, Q = index([Ring1]) = 1, l = 2 - 2 = 0: the double ring bond 0=2;
                                 the writer needs it as a tree bond: atom 2's tree bond is single, so its predecessor becomes 0
                                 with order 2 and 1-2 is the closure                                               C1=CC1
      [C][NH1][C]                cap([NH1]) = 3 - 1 = 2: o=1, s=1; a bracket atom with exactly the stated hydrogen C[NH]C
      [C][N+1][=Branch1][C][=O][O-1]   N+ cap 4: o=1, s=3; =Branch1: b = min(2, 2) = 2, Q=0: [=O] with o = min(2, 2, 2); resume s=1;
                                 [O-1] cap 1, o=1                                                                  C[N+](=O)[O-]
      [NH1][C]                   the first atom takes o=0, s=2; unused capacity stays unused                       [NH]C
      [C][C][Branch1][Ring1][C][C][C][O]   Q = index([Ring1]) = 1: the branch is [C][C]; then [C][O] on the main chain               CC(CC)CO
      [C][nop][C][=Branch1]      nop does nothing; =Branch1 at s=3 opens an empty branch at the row end            CC
      [C]<pad>[C], <pad>, [C]<unk>   a token that is no symbol: status 1 with its column (column 0 is <bos>)
      the empty row              status 1 at the <eos> column: no atom;  [nop][Ring1][Branch1]: symbols but no atom, status 1 at <eos>"""
    sv = VC.SelfiesVocab({s for row in HAND for s in SF.split(row[0]) if s.startswith("[")} | set(VC.SELFIES_INDEX_SYMBOLS))
    v = CR.vocabulary()
    out, out_len, status, info = decode_host(selfies_rows([r[0] for r in HAND], sv), sv)
    want = [r for r in HAND if r[1] is not None]
    c_out, c_len, c_st = canon_host([r[1] for r in want])
    assert (c_st == 0).all()
    k = 0
    for b, row in enumerate(HAND):
        if row[1] is None:
            assert status[b] == 1 and info[b].tolist() == [0, 0, 0, row[2]] and out_len[b] == 2, (row, status[b], info[b])
            assert out[b, :2].tolist() == [v.bos, v.eos] and (out[b, 2:] == v.pad).all()
            continue
        assert status[b] == 0 and same_row(out[b], out_len[b], c_out[k], c_len[k]), (row, status[b], smiles_text(out[b], out_len[b], v))
        assert info[b, 0] == len(SF.tree(row[1])[0]) and info[b, 3] == -1
        k += 1
    assert info[[r[0] for r in HAND].index("[C][C][C][=Ring1][Ring1]")].tolist() == [3, 1, 1, -1]
    # the reference derives the same table
    for row in want:
        st, atoms, _ = SF.derive(SF.split(row[0]))
        assert st == 0 and SF.spell(atoms) is not None
    r_out, r_len, r_st = canon_host([SF.spell(SF.derive(SF.split(r[0]))[1]) for r in want])
    assert (r_st == 0).all() and all(same_row(r_out[i], r_len[i], c_out[i], c_len[i]) for i in range(len(want)))


def random_rows(n=2000, seed=SEED):
    """n rows of symbols uniform over SelfiesVocab.default(), lengths uniform in 1 .. 127."""
    if "rand" not in _CACHE:
        sv = svocab()
        rs = np.random.RandomState(seed)
        rows = []
        for _ in range(n):
            rows.append([sv.symbols[i] for i in rs.randint(len(sv.symbols), size=int(rs.randint(1, 128)))])
        x = selfies_rows(["".join(r) for r in rows], sv, T=131)
        _CACHE["rand"] = (rows, x, decode_host(x, sv))
    return _CACHE["rand"]


def test_decode_host_equals_the_reference_on_random_rows():
    """2,000 random rows, symbols uniform over the default alphabet, lengths uniform in 1 .. 127.  Wherever the status is 0 the tokens
    are the canon host entry's spelling of the reference's graph; the statuses are 0 and 9 - 13, and 1 exactly where the reference finds no atom; every status-9 row has a ring bond
    of order >= 2 in the reference's graph; every output walks with status 0.  CPU figures: 1,996 of the 2,000 rows have status 0 (two have no atom, one is 9, one 12), 1,993 of them were compared."""
    rows, x, (out, out_len, status, info) = random_rows()
    v = CR.vocabulary()
    refs = [SF.derive(r) for r in rows]
    # The definition gives a row that adds no atom status 1, and a uniform draw of one to three symbols can be all ring, branch and nop
    # symbols: status 1 is taken exactly where the reference finds no atom, and nowhere else.
    assert np.array_equal(status == 1, np.array([r[0] == 1 for r in refs])) and all(len(rows[b]) <= 6 for b in np.nonzero(status == 1)[0])
    assert set(status.tolist()) <= {0, 1, 9, 10, 11, 12, 13}, np.bincount(status)
    assert [len(r[1]) for r in refs] == info[:, 0].tolist()
    for b in np.nonzero(status == 9)[0]:
        assert multiple_ring_bond(refs[b][1]), rows[b]
    ok = np.nonzero(status == 0)[0]
    spelled = [SF.spell(refs[b][1]) for b in ok]
    able = [i for i, s in enumerate(spelled) if s is not None and len(s) <= 127]
    assert len(able) >= 0.98 * len(ok), (len(able), len(ok))
    # the rows the kernel re-parented a multiple ring bond in are the ones a writer is likeliest to decline: all of them are compared
    moved = {int(b) for b in ok if info[b, 2] > 0}
    assert len(moved) >= 10 and moved <= {int(ok[i]) for i in able}, (len(moved), sorted(moved - {int(ok[i]) for i in able}))
    c_out, c_len, c_st = canon_host([spelled[i] for i in able])
    for j, i in enumerate(able):
        b = ok[i]
        assert c_st[j] == 0 and same_row(out[b], out_len[b], c_out[j], c_len[j]), (rows[b], spelled[i], smiles_text(out[b], out_len[b], v))
    ti, ci, _ = smiles_tables(v)
    g_status = ops.smiles_graph_host(torch.from_numpy(out[ok]), ti, ci, v.eos)[0].numpy()
    assert (g_status == 0).all()
    print("status histogram", np.bincount(status, minlength=14).tolist(), "comparable", len(able))
    assert len(ok) >= 0.9 * len(rows), len(ok)
    # a refused row is the empty row
    bad = status != 0
    assert (out_len[bad] == 2).all() and (out[bad, 0] == v.bos).all() and (out[bad, 1] == v.eos).all() and (out[bad, 2:] == v.pad).all()


def test_decode_host_equals_the_reference_on_ring_heavy_rows():
    """The uniform rows end their chains early and hold few multiple ring bonds, so 600 more rows are drawn from the symbols that make
    rings: carbon and nitrogen with single and double bonds, the four ring symbols, [Branch1].  Every status-0 row is compared token for
    token, none left out; 54 of them had a ring bond re-parented (15 rows are status 9); status 9 only where a bond on a cycle of the reference's graph has order >= 2 (a ring symbol's own bond, or a tree bond the
    writer's search would have to close a ring with)."""
    sv = svocab()
    rs = np.random.RandomState(SEED + 1)
    alphabet = ["[C]", "[C]", "[=C]", "[N]", "[=N]", "[O]", "[Ring1]", "[=Ring1]", "[Ring2]", "[=Ring2]", "[Branch1]"]
    rows = [[alphabet[i] for i in rs.randint(len(alphabet), size=int(rs.randint(4, 41)))] for _ in range(600)]
    out, out_len, status, info = decode_host(selfies_rows(["".join(r) for r in rows], sv), sv)
    refs = [SF.derive(r) for r in rows]
    assert np.array_equal(status == 1, np.array([r[0] == 1 for r in refs])) and set(status.tolist()) <= {0, 1, 9, 10, 11, 12, 13}
    for b in np.nonzero(status == 9)[0]:
        assert multiple_ring_bond(refs[b][1]), rows[b]
    ok = np.nonzero(status == 0)[0]
    spelled = [SF.spell(refs[b][1]) for b in ok]
    assert all(s is not None for s in spelled), [rows[ok[i]] for i, s in enumerate(spelled) if s is None][:3]
    c_out, c_len, c_st = canon_host(spelled)
    for j, b in enumerate(ok):
        assert c_st[j] == 0 and same_row(out[b], out_len[b], c_out[j], c_len[j]), (rows[b], spelled[j])
    print("ring-heavy rows: status", np.bincount(status, minlength=14).tolist(), "re-parented", int((info[ok, 2] > 0).sum()),
          "with ring bonds", int((info[ok, 1] > 0).sum()))
    assert (info[ok, 2] > 0).sum() >= 40 and (info[ok, 1] > 0).sum() >= 150 and len(ok) >= 500      # the input is not degenerate (found: 54, 218, 585)


EXTRA = ["CI(C)C", "FI(F)F", "C[C]C", "C[SH5]", "C[BH4-]", "C[C@H](N)O", "c1cccn1", "C" * 128, "C1CCC1(C)(C)C", "[N+2]C", "C1C1", "cc",
         "C[NH]C", "[CH3]C", "C[N]C", "[H]C", "C[O]", "C1CCCCCCCCCCCCCCCCCCC1", "C12(CCCCCCCCCCCCCCCCC1)CCCCCCCCCCCCCCCCCC2",
         "C1C2C3C4C5C6C7C8C9C0" + "C" * 87 + "C1C2C3C4C5C6C7C8C9C0"]      # 127 characters, 107 atoms and ten [Ring2] of three symbols: 137


def encode_cases():
    """(strings, the reference's (status, text) per row, the host entry's outputs)."""
    if "enc" not in _CACHE:
        rows = CR.mutation_corpus() + RR.fragment_corpus(100, seed=1) + [s for _, ks, a, _ in TA.TABLE for s in ks + [a]] + TA.STAY_KEKULE \
            + TA.NOT_AROMATIC + TA.NOT_KEKULE + [TA.EIGHT_RING] + EXTRA
        rows = list(dict.fromkeys(rows))
        sv = svocab()
        have = set(sv.symbols)
        refs = [SF.encode(s, m, have) for s, m in zip(rows, mates(rows))]
        _CACHE["enc"] = (rows, refs, encode_host(rows, sv, T=131))
    return _CACHE["enc"]


def test_encode_host_equals_the_reference():
    """The mutation corpus, 100 fragment rows, the aromatic hand tables and a few rows for the refusals: status and tokens equal the
    reference's, a refused row is the empty row, and every refusal 1 - 8, 12, 13 and 18 occurs (12 at max_content = 20 as well)."""
    rows, refs, (out, out_len, status, info) = encode_cases()
    sv = svocab()
    want = selfies_rows([t for _, t in refs], sv, T=out.shape[1])
    want_len = np.array([len(SF.split(t)) + 2 for _, t in refs], np.int32)
    want_st = np.array([st for st, _ in refs], np.int32)
    bad = np.nonzero(status != want_st)[0]
    assert len(bad) == 0, [(rows[b], int(status[b]), refs[b]) for b in bad[:10]]
    assert np.array_equal(out_len, want_len)
    bad = np.nonzero((out != want).any(1))[0]
    assert len(bad) == 0, [(rows[b], sv.ids2string(out[b, :out_len[b]].tolist()), refs[b][1]) for b in bad[:10]]
    assert (out_len[status != 0] == 2).all()
    seen = set(status.tolist())
    s_out, s_len, s_st, _ = encode_host(rows, sv, T=131, max_content=20)
    short = [SF.encode(s, m, set(sv.symbols), 20) for s, m in zip(rows, mates(rows))]
    assert np.array_equal(s_st, np.array([st for st, _ in short], np.int32)) and 12 in set(s_st.tolist())
    assert np.array_equal(s_out, selfies_rows([t for _, t in short], sv, T=s_out.shape[1]))
    assert seen >= {0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 13, 18}, sorted(seen)
    assert info[rows.index("CI(C)C")].tolist() == [4, 0, 0, 1] and info[rows.index("c1ccc2ccccc2c1")].tolist() == [10, 0, 2, -1]
    assert sv.ids2string(out[rows.index("c1cc[nH]c1")].tolist()[:9]) == "[C][C][=C][NH1][C][=Ring1][Branch1]"


ROUND_TRIP_FLOOR = 450                         # of the 494 rows with aromatize status 0 (CPU)


def test_round_trip_through_selfies_keeps_the_molecule():
    """For every row with encode status 0 and aromatize status 0: aromatize(decode(encode(x))) == aromatize(x), token for token, and the
    reference's derivation of encode(x) skips no branch and ends no chain early.  The rows that pass: ROUND_TRIP_FLOOR, found on the CPU,
    which is at least half of the rows with aromatize status 0."""
    rows, refs, (out, out_len, status, info) = encode_cases()
    sv, v = svocab(), CR.vocabulary()
    a_out, a_len, a_st = aromatize_host(CR.token_rows(rows, v))
    both = np.nonzero((status == 0) & (a_st == 0))[0]
    d_out, d_len, d_st, d_info = decode_host(out[both], sv)
    assert (d_st == 0).all(), [(rows[both[i]], int(d_st[i])) for i in np.nonzero(d_st)[0][:10]]
    assert np.array_equal(d_info[:, 0], info[both, 0])                     # the atoms
    b_out, b_len, b_st = aromatize_host(d_out)
    passed = 0
    for i, b in enumerate(both):
        assert b_st[i] == 0 and same_row(b_out[i], b_len[i], a_out[b], a_len[b]), (rows[b], smiles_text(b_out[i], b_len[i], v),
                                                                                    smiles_text(a_out[b], a_len[b], v))
        st, atoms, notes = SF.derive(SF.split(refs[b][1]))
        assert st == 0 and notes["skipped"] == 0 and notes["early"] == 0, (rows[b], refs[b][1], notes)
        passed += 1
    print("round trip", passed, "of", int((a_st == 0).sum()), "rows with aromatize status 0")
    assert passed >= ROUND_TRIP_FLOOR and 2 * passed >= int((a_st == 0).sum())


def test_selfies_vocab():
    sv = svocab()
    assert len(sv.symbols) <= 60 and len(sv) <= 64 and set(VC.SELFIES_INDEX_SYMBOLS) | {"[=Ring1]", "[=Ring2]", "[nop]"} <= set(sv.symbols)
    assert {"[F]", "[Cl]", "[Br]", "[I]", "[B]", "[S]", "[P]", "[N+1]", "[O-1]", "[NH1]"} <= set(sv.symbols)
    text = "[C][=C][Branch1][C][Cl][NH1+1][=Ring1][#Branch2][nop]"
    ids = sv.string2ids(text, add_bos=True, add_eos=True)
    assert ids[0] == sv.bos and ids[-1] == sv.eos and sv.unk not in ids and sv.ids2string(ids) == text
    assert sv.string2ids("[Se]") == [sv.unk]
    assert len({sv.c2i[c] for c in sv.c2i}) == len(sv) and sv.vectors.shape == (len(sv), len(sv))
    assert VC.SelfiesVocab.from_data(["[C][O]", "[C][=N]"]).symbols == ["[=N]", "[C]", "[O]"]
    with pytest.raises(ValueError):
        sv.string2ids("[C]C")
    info, emit = VC.selfies_info_table(sv), VC.selfies_emit_table(sv)
    assert info.dtype == emit.dtype == torch.int32 and info.shape == (len(sv),) and emit.shape == (529,)

    def word(sym):
        return int(info[sv.symbol2id(sym)])
    el = VC.SMI_ELEMENTS.index
    assert word("[C]") == 1 | 1 << 3 | el("C") << 5 | 1 << 9
    assert word("[=N]") == 1 | 2 << 3 | el("N") << 5 | 1 << 9 | 11 << 20
    assert word("[#C]") == 1 | 3 << 3 | el("C") << 5 | 1 << 9 | 13 << 20
    assert word("[NH1+1]") == 1 | 1 << 3 | el("N") << 5 | 2 << 9 | 1 << 11 | 1 << 12
    assert word("[O-1]") == 1 | 1 << 3 | el("O") << 5 | 0 << 9 | 1 << 11
    assert word("[=Branch2]") == 2 | 2 << 3 | 2 << 16 | 7 << 20 and word("[Ring1]") == 3 | 1 << 3 | 1 << 16 | 1 << 20
    assert word("[=Ring2]") == 3 | 2 << 3 | 2 << 16 and word("[nop]") == 4 | 1 << 3
    assert int(info[sv.eos]) == 5 and int(info[sv.bos]) == int(info[sv.pad]) == int(info[sv.unk]) == 0
    for v_, sym in enumerate(VC.SELFIES_INDEX_SYMBOLS):
        assert int(emit[513 + v_]) == sv.symbol2id(sym) and word(sym) >> 20 == v_
    assert int(emit[(((2 - 1) * 11 + el("N")) * 3 + 2) * 5 + 1]) == sv.symbol2id("[=NH1+1]")
    assert int(emit[495 + 1 * 3 + 0]) == sv.symbol2id("[=Branch1]") and int(emit[504 + 1 * 3 + 1]) == sv.symbol2id("[=Ring2]")
    assert int(emit[495 + 2]) == -1 and int(emit[(((1 - 1) * 11 + el("I")) * 3 + 2) * 5]) == -1          # [Branch3], [I+1]
    assert int((emit >= 0).sum()) == len(sv.symbols) - 1 + 16                                             # all but [nop], and the 16 index roles
    for bad in ("[Se]", "C", "[C", "[F+1]", "[I-1]x", "[F-1]", "[OH2]", "[IH1]", "[CH5]", "[N+2]", "[Branch4]", "[=nop]", "[c]"):
        with pytest.raises(ValueError):
            VC.SelfiesVocab(["[C]", bad])
    with pytest.raises(ValueError):
        VC.SelfiesVocab([f"[{b}{e}H{h}]" for b in ("", "=") for e in "CNBPS" for h in (1, 2)] + [f"[{b}{e}]" for b in ("", "=", "#") for e in ("C", "N", "O", "S", "P", "B", "F", "Cl", "Br", "I", "H")] + list(VC.SELFIES_INDEX_SYMBOLS) + ["[N+1]", "[O-1]", "[nop]", "[=Ring1]", "[=Ring2]", "[Ring3]", "[Branch3]"])


def test_entries_refuse_bad_arguments():
    sv, v = svocab(), CR.vocabulary()
    lib = L.load()
    x = torch.from_numpy(selfies_rows(["[C][O]"], sv, T=8))
    sinfo, emit = VC.selfies_info_table(sv), VC.smiles_emit_table(v)
    out, out_len, status = torch.empty(1, 8, dtype=torch.int64), torch.empty(1, dtype=torch.int32), torch.empty(1, dtype=torch.int32)
    p = ops.ptr

    def call(B=1, T=8, V=len(sv), ld=8, bos=v.bos, max_content=6, T_out=8, table=sinfo):
        return lib.mvae_selfies_decode_host(B, T, V, p(x), ld, p(table), p(emit), bos, v.eos, v.pad, max_content, T_out, p(out), p(out_len),
                                            p(status), None)
    assert call() == 0 and int(status[0]) == 0
    assert call(V=65) == -3
    for kw in (dict(B=0), dict(T=0), dict(ld=7), dict(bos=256), dict(bos=-1), dict(max_content=0), dict(max_content=128), dict(T_out=1),
               dict(table=None), dict(V=0)):
        assert call(**kw) == -1, kw
