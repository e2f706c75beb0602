"""CPU tests of the substructure search (mvae_smiles_substruct_compile_host / _rows / _corpus / _host): the host entry
(csrc/smiles_substruct.hip compiled for the CPU) against the reference of tests/substruct_ref.py, byte for byte in hit, undecided, map
and steps; the reference against networkx' monomorphism test and against an exhaustive search for the smallest embedding; five
deliberately broken references that those checks must catch; invariance under respelling; the step budget; the conditions the test
corpus has to meet; which queries compile; every refusal; the declarations and the compiler's resource remarks; the Python surface."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from molecular_vae_amd import _lib as L, vocab as VC, ops
import chem_ref as CR
import rewrite_ref as RR
import substruct_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mvae_smiles_substruct_compile_host", "mvae_smiles_substruct_rows", "mvae_smiles_substruct_corpus", "mvae_smiles_substruct_host")
NAMES = ("status", "hit", "undecided", "map", "steps")


def tables(v):
    return VC.smiles_token_table(v), VC.smiles_chem_table(v), VC.smiles_emit_table(v)


def compile_queries(queries, v=None, T=None):
    v = CR.vocabulary() if v is None else v
    tok, chem, emit = tables(v)
    return ops.smiles_substruct_compile(torch.from_numpy(CR.token_rows(queries, v, T)), tok, chem, emit, v.eos)


def host(strings, table, max_steps=SR.STEPS, map_query=None, v=None, T=None, **kw):
    v = CR.vocabulary() if v is None else v
    tok, chem, _ = tables(v)
    out = ops.smiles_substruct_host(torch.from_numpy(CR.token_rows(strings, v, T)), tok, chem, v.eos, table, max_steps, map_query, **kw)
    return tuple(None if t is None else t.numpy() for t in out)


def bits(words, Q):
    return ((words[:, None] >> np.arange(Q, dtype=np.int64)[None, :]) & 1).astype(bool)


def want_arrays(refs, nq, map_query):
    """The reference's (result, map, steps) per (row, query) as the arrays the entries write."""
    B, Q = len(refs), len(refs[0])
    res = np.array([[r[0] for r in row] for row in refs])
    steps = np.array([[r[2] for r in row] for row in refs], np.int32)
    weight = (np.uint64(1) << np.arange(Q, dtype=np.uint64))[None, :]
    hit = ((res == SR.HIT) * weight).sum(1, dtype=np.uint64).view(np.int64)
    und = ((res == SR.UNDECIDED) * weight).sum(1, dtype=np.uint64).view(np.int64)
    m = np.full((B, 32), 0xFF, np.uint8)
    for b, row in enumerate(refs):
        if row[map_query][0] == SR.HIT:
            m[b, :nq[map_query]] = row[map_query][1]
    return hit, und, m, steps


_CASES = {}


def cases():
    """(rows, their atoms, the queries' atoms, the reference's result per (row, query), the compiled table): computed once per process
    and shared; callers leave it unchanged."""
    if "c" not in _CASES:
        rows = SR.corpus()
        R, Q = [RR.atoms_of(s) for s in rows], [RR.atoms_of(q) for q in SR.QUERIES_22]
        table, qstatus = compile_queries(SR.QUERIES_22)
        assert not qstatus.any()
        _CASES["c"] = (rows, R, Q, [[SR.search(r, q) for q in Q] for r in R], table)
    return _CASES["c"]


def test_entries_are_declared_bound_and_exported_at_abi_12():
    text = open(os.path.join(ROOT, "include", "mvae.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert int(re.search(r"#define MVAE_ABI_VERSION (\d+)", header).group(1)) == 12 == L.ABI_VERSION
    lib = L.load()
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert len(L.SIGNATURES[ENTRIES[1]][1]) == len(L.SIGNATURES[ENTRIES[3]][1]) + 1 == 19
    for macro, value in (("QATOMS", ops.SUBSTRUCT_QATOMS), ("QUERIES", ops.SUBSTRUCT_QUERIES), ("WORDS", ops.SUBSTRUCT_WORDS),
                         ("MAX_STEPS", ops.SUBSTRUCT_MAX_STEPS)):
        assert int(re.search(r"#define\s+MVAE_SUBSTRUCT_" + macro + r"\s+(\d+)", header).group(1)) == value, macro
    assert (ops.SUBSTRUCT_QATOMS, ops.SUBSTRUCT_QUERIES, ops.SUBSTRUCT_STEPS) == (SR.QATOMS, SR.QUERIES, SR.STEPS) == (32, 64, 65536)
    assert int(re.search(r"#define\s+MVAE_SMILES_QUERY_ATOMS\s+(\d+)", header).group(1)) == ops.SMILES_STATUS_QUERY_ATOMS == SR.QUERY_ATOMS
    assert "SMILES substructure" in text and "NOT SMARTS" in text and "HasSubstructMatch" in text
    build = open(os.path.join(ROOT, "molecular-vae_amd", "csrc", "build.sh")).read()
    assert build.count(" smiles_substruct smiles_canon ") == 2 and "build/smiles_substruct.o build/smiles_canon.o" in build
    assert "build/tune/smiles_substruct.o build/tune/smiles_canon.o" in build
    # the adjacency is shared with the writer, not copied
    src = open(os.path.join(ROOT, "molecular-vae_amd", "csrc", "smiles_substruct.hip")).read()
    assert '#include "smiles_writer.hpp"' in src and "rew::adjacency(" in src and "rew::graph(" not in src


def test_new_kernels_use_no_scratch(tmp_path):
    """The compiler's resource remarks for the two kernels of smiles_substruct.hip: scratch 0, no spills, and the LDS per block that
    include/mvae.h states."""
    csrc = os.path.join(ROOT, "molecular-vae_amd", "csrc")
    usage = os.path.join(csrc, "build", "smiles_substruct.usage.txt")
    sources = ("smiles_substruct.hip", "smiles_writer.hpp", "smiles_rounds.hpp", "smiles_graph.hpp", "smiles_syntax.hpp", "common.hpp",
               "../../include/mvae.h")
    if os.path.exists(usage) and os.path.getmtime(usage) >= max(os.path.getmtime(os.path.join(csrc, f)) for f in sources):
        text = open(usage, errors="replace").read()
    else:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        run = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                              "-c", os.path.join(csrc, "smiles_substruct.hip"), "-o", str(tmp_path / "smiles_substruct.dev.o")],
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert run.returncode == 0, run.stderr[-2000:]
        text = run.stderr
    names = re.findall(r"Function Name: (\S+)", text)
    assert len(names) == 2 and all(any(k in n for n in names) for k in ("smiles_substruct_rows_kernel", "smiles_substruct_corpus_kernel")), names
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text) == ["0"] * 2
    assert re.findall(r"VGPRs Spill: (\d+)", text) == ["0"] * 2 and re.findall(r"SGPRs Spill: (\d+)", text) == ["0"] * 2
    header = open(os.path.join(ROOT, "include", "mvae.h")).read()
    stated = int(re.search(r"#define\s+MVAE_SUBSTRUCT_LDS_BYTES\s+(\d+)", header).group(1))
    assert list(map(int, re.findall(r"LDS Size \[bytes/block\]: (\d+)", text))) == [stated] * 2
    assert f"MVAE_SUBSTRUCT_LDS_BYTES = {stated} B" in header and stated <= 80 * 1024
    assert all(int(n) <= 128 for n in re.findall(r" VGPRs: (\d+)", text))


def test_host_entry_equals_the_reference_byte_for_byte():
    """hit, undecided and steps of all 1,027 x 22 pairs, and the map for each query in turn."""
    rows, R, Q, refs, table = cases()
    assert len(rows) == 1027 and len(Q) == 22
    nq = [len(q) for q in Q]
    for mq in range(len(Q)):
        status, hit, und, m, steps = host(rows, table, map_query=mq, T=131)
        w_hit, w_und, w_map, w_steps = want_arrays(refs, nq, mq)
        assert not status.any()
        wrong = [n for n, g, w in zip(NAMES[1:], (hit, und, m, steps), (w_hit, w_und, w_map, w_steps)) if not np.array_equal(g, w)]
        assert not wrong, (mq, wrong)
    bare = host(rows[:40], table, T=131, steps=False)
    assert bare[3] is None and bare[4] is None and np.array_equal(bare[1], hit[:40])


def test_conditions_on_the_test_corpus():
    """Asserted on the reference alone, so that a kernel that calls everything undecided, a hit or a miss cannot pass the comparison:
    nothing is undecided at the default budget, every query hits a row and misses a row."""
    rows, R, Q, refs, table = cases()
    res = np.array([[r[0] for r in row] for row in refs])
    steps = np.array([[r[2] for r in row] for row in refs])
    hits = (res == SR.HIT).sum(0)
    print("hits per query:", dict(zip(SR.QUERIES_22, hits.tolist())), "worst steps per query:", steps.max(0).tolist())
    assert not (res == SR.UNDECIDED).any() and steps.max() < SR.STEPS
    assert (hits >= 1).all() and (hits < len(rows)).all()
    assert steps.max() == 4529 and rows[int(steps.max(1).argmax())] == "C1CC1" * 25 + "CC"      # C1CCCCC1 on the 25 cyclopropanes


def test_reference_agrees_with_networkx_and_the_broken_variants_do_not():
    """Hit and miss of the reference equal networkx' subgraph_is_monomorphic with the same node and edge predicates, on every
    (row, query) of the set.  Four of the broken matchers disagree with networkx on a named (row, query).  The fifth, unsorted
    candidates, examines the same candidates in another order and so cannot differ in hit or miss: what it gets wrong is WHICH embedding
    comes first, and it is caught by the smallest embedding (which the fourth test holds the reference to)."""
    rows, R, Q, refs, table = cases()
    for b in range(len(rows)):
        for q in range(len(Q)):
            assert (refs[b][q][0] == SR.HIT) == SR.nx_monomorphic(R[b], Q[q]), (rows[b], SR.QUERIES_22[q])
    caught = {"ignores_bond_class": ("C1CCC2CCCCC2C1", "C=C"),     # (row, query) of this set: a single bond taken for a double one
              "not_injective": ("C1CC2(C1)CC2", "C1CCCCC1"),       # twice round a four-ring
              "ignores_closures": ("C1CCC2CCCCC2C1", "C1CC1"),     # a chain taken for a ring
              "ignores_charge": ("[O-]C(=O)C", "C(=O)O")}
    for broken, (row, query) in caught.items():
        assert row in rows and query in SR.QUERIES_22
        r, q = RR.atoms_of(row), RR.atoms_of(query)
        assert SR.search(r, q)[0] == SR.MISS and not SR.nx_monomorphic(r, q) and SR.search(r, q, broken=broken)[0] == SR.HIT, broken
    # unsorted candidates: the atom that closes the four-ring has the neighbours 2, 0, 4 in string order
    r, q = RR.atoms_of("C1CCC1C"), RR.atoms_of("C(C)(C)C")
    good, bad = SR.search(r, q), SR.search(r, q, broken="unsorted_candidates")
    assert good[:2] == (SR.HIT, [3, 0, 2, 4]) and good[1] == SR.smallest_embedding(r, q) and bad[:2] == (SR.HIT, [3, 2, 0, 4])
    for b in range(len(rows)):
        assert all(SR.search(R[b], Q[k], broken="unsorted_candidates")[0] == refs[b][k][0] for k in range(len(Q)))


def test_first_map_is_the_smallest_embedding():
    """Every map of the host entry is injective and satisfies rules 1 and 2; for every hit of a query of at most 6 atoms it is the
    smallest embedding found by exhaustive enumeration."""
    rows, R, Q, refs, table = cases()
    checked = small = 0
    for mq, q in enumerate(Q):
        _, hit, _, m, _ = host(rows, table, map_query=mq, T=131)
        got = bits(hit, len(Q))[:, mq]
        for b in np.nonzero(got)[0]:
            emb = m[b, :len(q)].tolist()
            assert SR.is_embedding(R[b], q, emb) and (m[b, len(q):] == 0xFF).all(), (rows[b], SR.QUERIES_22[mq])
            checked += 1
            if len(q) <= 6:
                assert emb == SR.smallest_embedding(R[b], q), (rows[b], SR.QUERIES_22[mq])
                small += 1
        assert (m[~got] == 0xFF).all()
    print("maps checked:", checked, "against the exhaustive search:", small)
    assert checked >= 1500 and small >= 1000


def test_respelling_changes_no_hit_bit_and_a_row_contains_itself():
    """Four respellings of every row by the host rewrite entry: the same hit bits; a row of at most 32 atoms without stereo, compiled as
    a query, hits itself and every respelling of itself."""
    rows, R, Q, refs, table = cases()
    v = CR.vocabulary()
    tok, chem, emit = tables(v)
    x = torch.from_numpy(CR.token_rows(rows, v, 131))
    base = host(rows, table, T=131)
    spelled = []
    for d in range(4):
        draws = ops.draw_words(torch.arange(len(rows)) * 4 + d)
        out, _, st = ops.smiles_rewrite_host(x, tok, chem, emit, v.bos, v.eos, v.pad, 7, draws, 127, 131)
        got = ops.smiles_substruct_host(out, tok, chem, v.eos, table)
        fine = (st == 0).numpy()
        assert fine.sum() >= 800                                        # the rewrite refuses the mutation corpus' stereo rows
        assert not got[0][fine].any() and not got[2].any()
        assert np.array_equal(got[1].numpy()[fine], base[1][fine])
        spelled.append((out, fine))
    # the check can fail: a matcher that reads the ROW without its ring-closure bonds depends on where the spelling closes its rings
    def tree_only(s):
        atoms = RR.atoms_of(s)
        pred = [next(iter(a["nb"]), None) for a in atoms]          # the first bond the string gave an atom is the one to its predecessor
        pred = [p if p is not None and p < k else None for k, p in enumerate(pred)]
        return [dict(a, nb={j: o for j, o in a["nb"].items() if pred[k] == j or pred[j] == k}) for k, a in enumerate(atoms)]
    out, fine = spelled[0]
    caught = 0
    for b in np.nonzero(fine)[0][:200]:
        ids = out[b].tolist()
        t = "".join(v.i2c[i] for i in ids[1:ids.index(v.eos)])
        assert all(SR.search(t, q)[0] == refs[b][k][0] for k, q in enumerate(Q)), (rows[b], t)
        a, c = tree_only(rows[b]), tree_only(t)
        caught += any(SR.search(a, q)[0] != SR.search(c, q)[0] for q in Q)
    print("rows on which a matcher without the row's closure bonds depends on the spelling:", caught)
    assert caught >= 1
    own = [b for b in range(len(rows)) if len(R[b]) <= 32 and not any(ch in rows[b] for ch in "@/\\")]
    assert len(own) >= 600
    for lo in range(0, len(own), 64):
        ids = own[lo:lo + 64]
        t, qs = compile_queries([rows[b] for b in ids], T=131)
        assert not qs.any()
        for rows_x, fine in [(x, np.ones(len(rows), bool))] + spelled:
            _, hit, und, _, _ = ops.smiles_substruct_host(rows_x[ids], tok, chem, v.eos, t)
            diag = bits(hit.numpy(), len(ids))[np.arange(len(ids)), np.arange(len(ids))]
            assert diag[fine[ids]].all() and not und.numpy()[fine[ids]].any()


def test_budget():
    """The 16-ring in 25 cyclopropanes: undecided at 65,536 steps, a miss at 131,072 after 92,938; steps equal the reference's."""
    table, qs = compile_queries([SR.BUDGET_QUERY, "C1CC1"])
    assert not qs.any()
    for budget, want in ((65536, SR.UNDECIDED), (131072, SR.MISS)):
        ref = SR.search(SR.BUDGET_ROW, SR.BUDGET_QUERY, budget)
        assert ref[0] == want and ref[2] == min(budget, 92938)
        status, hit, und, m, steps = host([SR.BUDGET_ROW, "CCO"], table, budget, 0)
        assert status.tolist() == [0, 0] and hit.tolist() == [2, 0] and und.tolist() == [int(want == SR.UNDECIDED), 0]
        assert steps.tolist() == [[ref[2], 4], [0, 0]] and (m == 0xFF).all()
    # a search that ends on its last allowed step is decided: C, C-C; C, C-C, C-C; C, C-C, C-O
    assert SR.search("CCCO", "CO", 8) == (SR.HIT, [2, 3], 8) and SR.search("CCCO", "CO", 7) == (SR.UNDECIDED, None, 7)
    t, _ = compile_queries(["CO"])
    for budget, want in ((8, ([1], [0], [[8]])), (7, ([0], [1], [[7]]))):
        got = host(["CCCO"], t, budget)
        assert (got[1].tolist(), got[2].tolist(), got[4].tolist()) == want


def test_query_handling():
    """AROMATIC-status fragments compile and match; stereo, 33 atoms, a syntax error and a valence error are refused with their reason
    and a table that matches nothing; [nH] matches any aromatic n, [H] only an explicit [H]."""
    queries = ["cC(=O)O", "c[N+](=O)[O-]", "C[C@H](N)O", "F/C=C/F", "C" * 33, "C" * 32, "C(", "C=F", "[nH]", "[H]", "n", "C"]
    assert [CR.analyse(q)[0] for q in queries[:2]] == [5, 5]
    table, qs = compile_queries(queries)
    assert qs.tolist() == [SR.query_status(q) for q in queries] == [0, 0, 8, 8, 14, 0, 1, 2, 0, 0, 0, 0]
    refused = qs.numpy() != 0
    assert not table.numpy()[refused].any() and (table.numpy()[~refused, 0] == [4, 4, 32, 1, 1, 1, 1]).all()
    rows = ["OC(=O)c1ccccc1", "c1ccccc1[N+](=O)[O-]", "CC(=O)O", "C" * 40, "c1cc[nH]c1", "c1ccncc1", "[H]C", "CC", "C[C@H](N)O"]
    status, hit, und, _, steps = host(rows, table)
    got = bits(hit, len(queries))
    want = np.array([[SR.search(r, q)[0] == SR.HIT if not bad else False for q, bad in zip(queries, refused)] for r in rows])
    assert not status.any() and not und.any() and np.array_equal(got, want) and not steps[:, refused].any()
    assert got[0, 0] and got[1, 1] and not got[2, 0] and got[3, 5] and not got[:, refused].any()
    assert got[4, 8] and got[5, 8] and got[4, 10] and got[6, 9] and not got[7, 9] and got[8, 11]      # a row with '@' is searched


def test_refusals_come_before_anything_is_written():
    lib = L.load()
    fake = ctypes.c_void_p(256)                                  # never dereferenced: every call below is refused first

    def rows(name, B=4, T=8, V=29, x=fake, ld=8, tok=fake, chem=fake, eos=1, Q=3, table=fake, ms=100, mq=0, status=fake, hit=fake,
             und=fake, m=None):
        tail = (None,) if name == ENTRIES[1] else ()
        return getattr(lib, name)(B, T, V, x, ld, tok, chem, eos, Q, table, ms, mq, status, hit, und, m, None, None, *tail)
    for name in (ENTRIES[1], ENTRIES[3]):
        assert rows(name, B=0) == -1 and rows(name, T=0, ld=0) == -1 and rows(name, V=0, eos=0) == -1 and rows(name, V=65) == -3
        assert rows(name, x=None) == -1 and rows(name, tok=None) == -1 and rows(name, chem=None) == -1 and rows(name, ld=7) == -1
        assert rows(name, eos=29) == -1 and rows(name, eos=-1) == -1 and rows(name, V=65, table=None) == -3
        assert rows(name, Q=0) == -1 and rows(name, Q=65) == -1 and rows(name, table=None) == -1 and rows(name, status=None) == -1
        assert rows(name, hit=None) == -1 and rows(name, und=None) == -1 and rows(name, ms=0) == -1 and rows(name, ms=(1 << 20) + 1) == -1
        assert rows(name, m=fake, mq=3) == -1 and rows(name, m=fake, mq=-1) == -1

    def corpus(tokens=fake, offsets=fake, N=100, V=29, tok=fake, chem=fake, Q=3, table=fake, ms=100, mq=0, status=fake, hit=fake, und=fake,
               m=None):
        return lib.mvae_smiles_substruct_corpus(tokens, offsets, N, V, tok, chem, Q, table, ms, mq, status, hit, und, m, None, None, None)
    assert corpus(N=0) == -1 and corpus(V=0) == -1 and corpus(V=65) == -3 and corpus(tokens=None) == -1 and corpus(offsets=None) == -1
    assert corpus(tok=None) == -1 and corpus(chem=None) == -1 and corpus(Q=0) == -1 and corpus(Q=65) == -1 and corpus(table=None) == -1
    assert corpus(status=None) == -1 and corpus(hit=None) == -1 and corpus(und=None) == -1 and corpus(ms=0) == -1
    assert corpus(ms=(1 << 20) + 1) == -1 and corpus(m=fake, mq=3) == -1 and corpus(N=1 << 40) == -3

    def comp(Q=3, T=8, V=29, x=fake, ld=8, tok=fake, chem=fake, eos=1, table=fake, qs=fake):
        return lib.mvae_smiles_substruct_compile_host(Q, T, V, x, ld, tok, chem, 0, 0, eos, table, qs)
    assert comp(Q=0) == -1 and comp(Q=65) == -1 and comp(V=65) == -3 and comp(x=None) == -1 and comp(table=None) == -1 and comp(qs=None) == -1
    assert comp(ld=7) == -1 and comp(eos=29) == -1 and comp(tok=None) == -1 and comp(chem=None) == -1
    # a refused call through the wrappers leaves prefilled outputs as they were
    table, _ = compile_queries(["CO", "CC"])
    v = CR.vocabulary()
    tok, chem, _ = tables(v)
    x = torch.from_numpy(CR.token_rows(["CCO"], v))
    pre = torch.full((1,), 77, dtype=torch.int64)
    with pytest.raises(ValueError, match=r"max_steps must be in \[1, 1048576\]"):
        ops.smiles_substruct_host(x, tok, chem, v.eos, table, 0, hit=pre)
    with pytest.raises(ValueError, match=r"map_query must be in \[0, 2\)"):
        ops.smiles_substruct_host(x, tok, chem, v.eos, table, 10, 2, hit=pre)
    with pytest.raises(L.MvaeError, match="mvae_smiles_substruct_host"):
        ops.smiles_substruct_host(x, tok, chem, len(v), table, hit=pre)
    assert pre.tolist() == [77]


def test_output_edges():
    """Prefilled outputs are fully overwritten; a strided x works; rows without <eos> and with ids outside the vocabulary are refused as
    the graph entry refuses them and hit nothing; counts accumulates; Q = 64 sets bit 63."""
    v = CR.vocabulary()
    tok, chem, _ = tables(v)
    queries = ["C"] * 63 + ["N"]
    table, qs = compile_queries(queries)
    assert not qs.any()
    strings = ["c1cccn1", "c1ccccc1", "C=F", "c1ccncc1", "CC(C)CN", "CCO"]
    x = torch.from_numpy(CR.token_rows(strings, v, T=12))
    x[0, 8] = v.pad                                                # no <eos>
    x[1, 3] = -1
    x[3, 2] = len(v)
    wide = torch.full((6, 40), v.eos, dtype=torch.long)
    wide[:, :12] = x
    pre = (torch.full((6,), 0x7f7f7f7f, dtype=torch.int32), torch.full((6,), 0x7f7f7f7f7f7f7f7f, dtype=torch.int64),
           torch.full((6,), 0x7f7f7f7f7f7f7f7f, dtype=torch.int64), torch.full((6, 32), 0x7f, dtype=torch.uint8),
           torch.full((6, 64), 0x7f7f7f7f, dtype=torch.int32))
    counts = torch.full((64, 2), 5, dtype=torch.int32)
    got = ops.smiles_substruct_host(wide[:, :12], tok, chem, v.eos, table, 65536, 63, *pre, counts=counts)
    graph = ops.smiles_graph_host(wide[:, :12], tok, chem, v.eos)[0]
    assert torch.equal(got[0], graph) and got[0].tolist() == [1, 1, 2, 1, 0, 0]
    assert got[1].tolist() == [0, 0, 0, 0, -1, (1 << 63) - 1] and not got[2].any() and got[1].dtype == torch.int64
    assert (got[3][:4] == 0xFF).all() and got[3][4].tolist() == [4] + [0xFF] * 31 and (got[3][5] == 0xFF).all()
    assert not got[4][:4].any() and got[4][4].tolist() == [1] * 63 + [5] and got[4][5].tolist() == [1] * 63 + [0]
    assert counts[:, 0].tolist() == [7] * 63 + [6] and counts[:, 1].tolist() == [5] * 64
    fresh = ops.smiles_substruct_host(wide[:, :12], tok, chem, v.eos, table, 65536, 63)
    assert all(torch.equal(a, b) for a, b in zip(fresh, got))
    # a table the compile entry did not write: every index is masked, the results mean nothing and the call returns
    rs = np.random.RandomState(0)
    junk = torch.from_numpy(rs.randint(-2 ** 31, 2 ** 31, size=(8, 100)).astype(np.int32))
    junk[:, 0] = torch.tensor([1, 2, 5, 32, 33, -1, 7, 31])
    junk[:, 1:4] = 0
    out = ops.smiles_substruct_host(torch.from_numpy(CR.token_rows(SR.corpus()[:64], v)), tok, chem, v.eos, junk, 1000, 3)
    assert int(out[4].max()) <= 1000 and not out[4][:, 4:6].any()


def test_python_surface():
    """data.compile_substructures and its refusals; VAE.has_substructure and the dataset methods raise on the CPU before any device
    work: no fallback; moses_generate's filter statistics recomputed from the samples it returns, with the reference."""
    import inspect
    from molecular_vae_amd import data as D, mosesvae as MV, train as TR
    v = CR.vocabulary()
    t = D.compile_substructures(["C(=O)O", "cC(=O)O", "C#N"], v)
    assert isinstance(t, D.SubstructureTable) and t.patterns == ("C(=O)O", "cC(=O)O", "C#N") and len(t) == 3
    assert t.table.shape == (3, 100) and t.table.dtype == torch.int32 and t.qstatus.tolist() == [0, 0, 0]
    assert torch.equal(t.table, compile_queries(["C(=O)O", "cC(=O)O", "C#N"])[0]) and D.compile_substructures(t, v) is t
    for bad, why in (("C[C@H](N)O", "stereo"), ("C" * 33, "query_atoms"), ("C(", "syntax"), ("C=F", "valence")):
        with pytest.raises(ValueError, match=re.escape(repr(bad)) + ".*" + why):
            D.compile_substructures(["CC", bad], v)
    with pytest.raises(ValueError, match="1 to 64 patterns"):
        D.compile_substructures([], v)
    with pytest.raises(ValueError, match="1 to 64 patterns"):
        D.compile_substructures(["C"] * 65, v)
    with pytest.raises(ValueError, match="not in the vocabulary"):
        D.compile_substructures(["C?"], v)
    torch.manual_seed(0)
    model = MV.VAE(VC.OneHotVocab(list("CNOc(=)1")), dtype=torch.float32)
    ds = D.MosesDeviceDataset(["CCO", "c1ccccc1"], model.vocabulary, device="cpu")
    with pytest.raises(L.MvaeError, match="MI355X only"):
        model.has_substructure(["CCO"], ["CO"])
    with pytest.raises(L.MvaeError, match="MI355X only"):
        ds.substructure_counts(["CO"])
    with pytest.raises(L.MvaeError, match="MI355X only"):
        ds.rows_with_substructure("CO")
    assert inspect.signature(TR.moses_generate).parameters["filters"].default is None
    assert inspect.signature(MV.VAE.has_substructure).parameters["max_steps"].default == 65536
    with pytest.raises(ValueError, match="'C\\('.*syntax"):
        TR.moses_generate(model, 4, filters=["C("])
    for bad in (0, (1 << 20) + 1, 2.5):
        with pytest.raises(ValueError, match="filter_steps must be an integer"):
            TR.moses_generate(model, 4, filters=["CO"], filter_steps=bad)
    # the statistics moses_generate derives from the device's hit and undecided words, on the host entry's words for the same strings
    strings = RR.fragment_corpus(40, seed=9) + ["C(", "C=F"]
    filters = ["C(=O)[O-]", "C#N", "S(=O)(=O)", "I"]
    ft = D.compile_substructures(filters, v)
    tok, chem, _ = tables(v)
    status, hit, und, _, _ = ops.smiles_substruct_host(torch.from_numpy(CR.token_rows(strings, v)), tok, chem, v.eos, ft.table)
    stats = TR.filter_statistics(status, hit, und, len(filters))
    fine = [s for s in strings if CR.analyse(s)[0] == 0]
    res = [[SR.search(s, q)[0] for q in filters] for s in fine]
    assert stats["filter_hits"] == [sum(r[k] == SR.HIT for r in res) for k in range(4)] and stats["filter_undecided"] == [0] * 4
    assert stats["filters"] == sum(all(x == SR.MISS for x in r) for r in res) / len(fine) and 0 < stats["filters"] < 1
    assert stats["filter_hits"][3] == 0 and min(stats["filter_hits"][:3]) >= 1
