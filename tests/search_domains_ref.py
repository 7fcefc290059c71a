"""Option "search_domains" restated on the host: the one definition of include/dmpfold_hip.h.

    gather by label -> test_align_cpu.yardstick on the gathered trace -> scatter -> rank by the stated rule

Pair (d, k) is what "align_structure" gives for a model consisting of exactly the rows of domain d, in rising order, and
entry k; its ali and deviation go back to the residues of the domain; rank[d] is the host's sort of the float32 tm_model.

    pair(model, labels, d, structure)    -> (the yardstick's dict on the domain, margin, the domain's residues)
    search(model, labels, D, library)    -> the whole answer as a dict, every pair through the yardstick
    block(L, answer)                     -> the domain-search block ((400 + 2L) K floats) that answer stands for

No GPU, no library."""
import numpy as np

from dmpfold2_amd import score as S
from test_align_cpu import yardstick

HEADER = S.ALIGN_HEADER


def residues(labels, d):
    """The residues of domain d in rising order."""
    return np.flatnonzero(np.asarray(labels).reshape(-1) == d)


def gather(model, labels, d):
    """The trace of domain d: the C-alpha rows i with labels[i] == d, in rising i (float32 (n_d, 3))."""
    return np.ascontiguousarray(np.asarray(model, dtype=np.float32).reshape(-1, 3)[residues(labels, d)])


def pair(model, labels, d, structure):
    want, margin = yardstick(gather(model, labels, d), structure)
    return want, margin, residues(labels, d)


def header_of(want):
    """The 24 header floats of a yardstick dict (offsets 1 .. 24 of an align block), float64."""
    h = np.zeros(HEADER)
    h[0], h[1], h[2], h[3] = want["n_ali"], want["rmsd_ali"], want["tm_model"], want["tm_struct"]
    h[4:13] = np.asarray(want["R"]).reshape(-1)
    h[13:16] = want["t"]
    h[16], h[17], h[18], h[19] = want["d0_model"], want["d0_struct"], want["seed_offset"], want["seeds"]
    return h


def search(model, labels, D, library, pairs=None):
    """Every pair (d, k), d < D, of a library (score.Library) - or only those of `pairs` (the rest NaN) - -> dict: headers
    (16, K, 24), ali (K, L), deviation (K, L), margins (D, K), rank (16, K) with NaN rows for d >= D (the sort of the float32
    tm_model by score.host_rank), wants {(d, k): the yardstick's dict}."""
    labels = np.asarray(labels).reshape(-1)
    L, K = labels.shape[0], len(library)
    headers = np.full((S.DOMAINS_MAX, K, HEADER), np.nan)
    ali = np.full((K, L), np.nan)
    dev = np.full((K, L), np.nan)
    margins = np.full((D, K), np.nan)
    wants = {}
    for d in range(D):
        for k in range(K):
            if pairs is not None and (d, k) not in pairs:
                continue
            want, margin, idx = pair(model, labels, d, library.entry(k))
            wants[d, k], margins[d, k] = want, margin
            headers[d, k] = header_of(want)
            ali[k, idx] = want["ali"]                      # the domains partition the chain: each residue is written once
            dev[k, idx] = want["deviation"]
    rank = np.full((S.DOMAINS_MAX, K), np.nan)
    for d in range(D):
        rank[d] = S.host_rank(headers[d, :, 2].astype(np.float32))
    return {"headers": headers, "ali": ali, "deviation": dev, "margins": margins, "rank": rank, "wants": wants}


def block(L, answer):
    """The domain-search block that `search`'s answer stands for (float32; each value rounded once)."""
    K = answer["ali"].shape[0]
    return S.pack_domain_search(L, K, answer["rank"], answer["headers"], answer["ali"], answer["deviation"])


def hit_of(ds, d, k, labels):
    """Pair (d, k) of score.unpack_domain_search in the shape test_align_cpu.compare_alignment takes: the header's fields,
    ali and deviation of the domain's residues in rising order."""
    idx = residues(labels, d)
    return dict(ds["hits"][d][k], ali=ds["ali"][k][idx], deviation=ds["deviation"][k][idx])
