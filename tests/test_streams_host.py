"""CPU tests of the stream registry (tests/stream_cases.py) against include/wats_hip.h: every prototype that takes
a `void* stream` is named by exactly one case or is excluded with a reason, the registry names nothing the header
lacks, and each class is what the doc comment above the prototype says.  A new stream-taking entry point fails
here until it is classified; tests/test_streams.py then holds it to its class on the GPU."""
import os
import re

import pytest

from conftest import REPO

import stream_cases as SC

HEADER = os.path.join(REPO, "include", "wats_hip.h")
# a prototype as tests/test_host.py's export check finds it, with its argument list
PROTOTYPE = re.compile(r"^\s*(?:const\s+char\s*\*|int)\s+(wg_\w+)\s*\(([^;{]*?)\)\s*;", re.M | re.S)
# a doc comment opens a line; the comments inside an argument list or behind a #define do not
DOC_COMMENT = re.compile(r"^/\*.*?\*/", re.M | re.S)


def header_prototypes(src=None):
    """name -> (arguments, the doc comment above the prototype) for every function of the header"""
    src = open(HEADER).read() if src is None else src
    docs = [(m.end(), m.group(0)) for m in DOC_COMMENT.finditer(src)]
    # blank the comments that do not open a line (same offsets): one of them holds a semicolon
    code = re.sub(r"(?<=[^\n])/\*.*?\*/", lambda m: " " * len(m.group(0)), src, flags=re.S)
    out = {}
    for m in PROTOTYPE.finditer(code):
        above = [text for end, text in docs if end <= m.start()]
        out[m.group(1)] = (m.group(2), above[-1] if above else "")
    return out


def stream_entries(src=None):
    return {name: doc for name, (args, doc) in header_prototypes(src).items() if re.search(r"void\s*\*\s*stream\b", args)}


def classified():
    """name -> the cases that name it"""
    owners = {}
    for c in SC.CASES:
        for name in c.names:
            owners.setdefault(name, []).append(c.name)
    return owners


def unclassified(src=None):
    return sorted(set(stream_entries(src)) - set(classified()) - set(SC.EXCLUDED))


def test_the_parser_sees_the_header():
    protos = header_prototypes()
    import ctypes
    from wats_hip import _lib
    assert set(protos) == set(_lib.SIGNATURES)                       # the same set test_host.py's check reads
    entries = stream_entries()
    assert len(entries) >= 56 and "wg_last_error" not in entries and "wg_chain_status" not in entries
    for name in entries:                                             # and the binding passes a pointer for it
        res, args = _lib.SIGNATURES[name]
        assert ctypes.c_void_p in args[-2:], name
    assert "scipy semantics" in entries["wg_column_degree"]          # the comment above, not one inside a prototype
    assert "wg_csr_patch (commit)" in entries["wg_csr_patch"] and "NULL = 1" not in entries["wg_laplacian_create"]


def test_every_stream_taking_prototype_is_classified_once():
    owners = classified()
    assert unclassified() == [], "classify these in tests/stream_cases.py (a case, or EXCLUDED with a reason)"
    twice = {name: cs for name, cs in owners.items() if len(cs) > 1}
    assert not twice, f"named by more than one case: {twice}"
    both = sorted(set(owners) & set(SC.EXCLUDED))
    assert not both, f"named by a case and excluded: {both}"
    assert all(isinstance(r, str) and r.strip() for r in SC.EXCLUDED.values())


def test_the_registry_names_nothing_the_header_lacks():
    entries = stream_entries()
    for name in list(classified()) + list(SC.EXCLUDED) + list(SC.ASYNC_REASONS):
        assert name in entries, f"{name} is not a stream-taking prototype of the header"
    assert len({c.name for c in SC.CASES}) == len(SC.CASES)
    for c in SC.CASES:
        assert c.klass in (SC.CAPTURABLE, SC.ASYNC, SC.SYNCHRONOUS) and c.names, c
        assert callable(c.make) and callable(c.run)
        assert not c.stateful or c.klass != SC.SYNCHRONOUS
    assert set(SC.ABI_PROBES) <= {c.name for c in SC.CASES}


def test_a_new_stream_taking_prototype_fails_until_it_is_classified():
    src = open(HEADER).read()
    added = src.replace("#ifdef __cplusplus\n}\n#endif\n#endif /* WATS_HIP_H */",
                        "int wg_new_entry(int64_t n, const float* x, float* y, void* stream);\n"
                        "#ifdef __cplusplus\n}\n#endif\n#endif /* WATS_HIP_H */")
    assert added != src
    assert unclassified(added) == ["wg_new_entry"]
    no_stream = added.replace("float* y, void* stream);", "float* y);")
    assert unclassified(no_stream) == []


@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c.name)
def test_the_class_is_the_headers_own_word(case):
    entries = stream_entries()
    for name in case.names:
        doc = entries[name]
        if case.klass == SC.CAPTURABLE:
            assert "captur" in doc, f"{name}: the header does not promise that it may be captured"
        elif case.klass == SC.SYNCHRONOUS:      # the word itself, not the tail of "asynchronous"
            assert re.search(r"(?<![Aa])[Ss]ynchronous", doc), f"{name}: the header does not call it synchronous"
        else:
            assert SC.ASYNC_REASONS.get(name, "").strip(), f"{name} is ASYNC without a stated reason"


def test_async_reasons_belong_to_async_cases():
    is_async = {name for c in SC.CASES if c.klass == SC.ASYNC for name in c.names}
    assert set(SC.ASYNC_REASONS) == is_async


def test_the_header_points_to_the_tests():
    opening = open(HEADER).read().split("#ifndef WATS_HIP_H")[0]
    assert "tests/test_streams.py" in opening and "tests/stream_cases.py" in opening
