"""What the track tests share: the fixture of tests/golden/make_track_golden.py (the reference's WiggleReader and
GenomeArray over small texts) and the comparisons."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

_fixture = None


def fixture():
    """(manifest, arrays) of tests/golden/track_fixture.npz, loaded once."""
    global _fixture
    if _fixture is None:
        z = np.load(os.path.join(HERE, "golden", "track_fixture.npz"))
        _fixture = (json.loads(str(z["manifest"])), {k: z[k] for k in z.files if k != "manifest"})
    return _fixture


def case_names():
    return [c["name"] for c in fixture()[0]["cases"]]


def refused_names():
    return [r["name"] for r in fixture()[0]["refused"]]


def case(name):
    return [c for c in fixture()[0]["cases"] if c["name"] == name][0]


def refused(name):
    return [r for r in fixture()[0]["refused"] if r["name"] == name][0]


def same_bits(a, b):
    """Bit for bit (the sign of zero included), any NaN equal to any NaN."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    if not np.array_equal(nan, np.isnan(b)):
        return False
    return np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def expected_tuples(c):
    return [tuple(t) for add in c["tuples"] for t in add]


def same_tuples(got, exp):
    if len(got) != len(exp):
        return False
    return all(g[0] == e[0] and g[1] == e[1] and g[2] == e[2] and same_bits([g[3]], [e[3]]) for g, e in zip(got, exp))


def sum_bound(arrays, c):
    """2 * n_nonzero * 2^-53 * sum |x| over the case's arrays: the textbook bound for reordering a float sum."""
    nnz, total = 0, 0.0
    for ch in c["chroms"]:
        for st in ("+", "-"):
            a = arrays["%s|%s|%s" % (c["name"], ch, st)]
            nnz += int(np.count_nonzero(a))
            total += float(np.abs(a).sum())
    return 2.0 * nnz * 2.0 ** -53 * total
