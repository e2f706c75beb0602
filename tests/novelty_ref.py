"""Reference of the corpus index (mvae_corpus_index_build / mvae_corpus_index_probe): a Python dict from a row's content, as a tuple of
ids, to the lowest corpus row that holds it, and the cut of a sampled token row that include/mvae.h states.  No hashing of ours and no
floats: every comparison against it is exact.  tests/test_moses_novelty_host.py pins it to plain ``in`` on a set of strings."""


def index(seqs):
    """seqs: the corpus rows' ids (without specials), in corpus order -> {tuple(ids): lowest row}."""
    table = {}
    for r, s in enumerate(seqs):
        table.setdefault(tuple(int(t) for t in s), r)
    return table


def content(row, eos):
    """A token row with <bos> in column 0 -> its content: row[1:] up to, and not including, the first `eos`; all of row[1:] without one."""
    out = []
    for t in list(row)[1:]:
        if int(t) == eos:
            break
        out.append(int(t))
    return tuple(out)


def lookup(table, rows, eos):
    """What the probe answers for every token row: the lowest corpus row with the row's content, -1 for none.  An id that is no uint8 is
    simply a key the table lacks."""
    return [table.get(content(r, eos), -1) for r in rows]


def n_distinct(table):
    return len(table)
