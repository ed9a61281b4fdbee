"""A claim of capturability in include/solo_mi355x.h cannot go untested: every function declared under a comment that speaks of capture is
named in the table of tests/test_gpu_graph_replay.py -- with the test that captures it, or with the reason why it is not captured."""
import ast
import os
import re

import solo_testlib as T

HEADER = os.path.join(T.ROOT, "include", "solo_mi355x.h")
MODULE = os.path.join(T.ROOT, "tests", "test_gpu_graph_replay.py")


def claims(text):
    """-> [(the functions declared between a comment that contains "captur" and the next comment, the comment's first line)]; a comment
    is one that begins its line -- the remarks behind a declaration or a struct field do not end the reach of the comment above them"""
    out = []
    blocks = [m for m in re.finditer(r"/\*.*?\*/", text, flags=re.S) if not text[text.rfind("\n", 0, m.start()) + 1:m.start()].strip()]
    for blk, nxt in zip(blocks, blocks[1:] + [None]):
        if "captur" not in blk.group(0).lower():
            continue
        code = text[blk.end():nxt.start() if nxt else len(text)]
        code = re.sub(r"/\*.*?\*/", "", code, flags=re.S)
        out.append((re.findall(r"\b(solo_\w+|AGR_\w+)\s*\(", code), blk.group(0).splitlines()[0]))
    return out


def tables():
    """CAPTURED and NOT_CAPTURED of the GPU module (imported: the module needs no GPU to load) and the names of its tests"""
    import test_gpu_graph_replay as M
    tests = {n.name for n in ast.parse(open(MODULE).read()).body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    return M.CAPTURED, M.NOT_CAPTURED, tests


def test_the_parser_finds_declarations():
    text = "/* a */ int32_t solo_a(int x);\n/* can be captured\n in a graph */\ntypedef struct { int a, b; } solo_t;\n#define SOLO_X 1\n" \
           "solo_t *solo_b(void);\nint32_t solo_c(solo_t *t,\n   void *s);\n/* next */ void solo_d(void);\n/* Captured too */ int solo_e(void);"
    assert claims(text) == [(["solo_b", "solo_c"], "/* can be captured"), (["solo_e"], "/* Captured too */")]


def test_every_claim_of_the_header_names_a_test():
    captured, not_captured, tests = tables()
    found = claims(open(HEADER).read())
    names = [f for fs, _ in found for f in fs]
    assert len(found) >= 10 and "solo_mix" in names and "solo_batch_encode" in names and "solo_agc" in names
    missing = [(f, first) for fs, first in found for f in fs if f not in captured and f not in not_captured]
    assert not missing, "declared under a comment that speaks of capture, but in neither table of tests/test_gpu_graph_replay.py: %s" % missing
    assert not set(captured) & set(not_captured)
    declared = set(re.findall(r"\b(solo_\w+)\s*\(", T.header_text()))
    assert set(captured) <= declared and set(not_captured) <= declared
    assert set(captured.values()) <= tests, sorted(set(captured.values()) - tests)
    assert all(isinstance(r, str) and r for r in not_captured.values())
