"""The call table of tests/stream_cases.py against the header, the binding and csrc/engine.hip (no GPU).

A call added to the header with a `stream` parameter and no row fails here; so does a row whose class is not what
engine.hip does: the class's HIP calls are looked up in the entry point's body and, through the file's own functions
it calls, in theirs."""
import inspect
import os
import re

from stream_cases import CALLS, NO_STREAM, REACHES, WAITS
from test_abi import prototypes

from libzombsole_amd import _abi
from libzombsole_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def takes_stream(params):
    return any(re.fullmatch(r"void\s*\*\s*stream", p) for p in params)


def test_the_table_is_the_prototypes_that_take_a_stream():
    protos = prototypes()
    with_stream = {n for n, p in protos.items() if takes_stream(p)}
    assert with_stream == set(CALLS), sorted(with_stream ^ set(CALLS))
    assert len(with_stream) == 33
    assert set(NO_STREAM) <= set(protos) - with_stream
    for name in with_stream:  # the stream is the last parameter, and the binding passes it as a pointer
        assert takes_stream(protos[name][-1:]) and _abi.ABI[name][-1] is _abi._vp, name
    for name, (cls, _) in list(CALLS.items()) + list(NO_STREAM.items()):
        assert cls in REACHES, (name, cls)
    assert {c for c, _ in CALLS.values()} == {"async", "sync", "first-call-sync"}


def test_every_row_names_the_engine_method_that_reaches_it():
    for name, (_, method) in list(CALLS.items()) + list(NO_STREAM.items()):
        src = inspect.getsource(getattr(Engine, method))
        assert '"%s"' % name in src, (name, method)
        if name in CALLS:  # ... and hands over the current stream
            assert "self._stream()" in src, (name, method)


def engine_functions():
    """{name: body text} of every function defined at column 0 of engine.hip (static helpers and extern "C" entry points)."""
    src = open(os.path.join(ROOT, "libzombsole_amd", "csrc", "engine.hip")).read()
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    heads = list(re.finditer(r'^(?:extern "C" |static |template [^\n]*\nstatic )[^\n;{]*?\b(\w+)\s*\([^;{]*\)\s*\{', src, re.M))
    out = {}
    for k, m in enumerate(heads):
        end = heads[k + 1].start() if k + 1 < len(heads) else len(src)
        out[m.group(1)] = out.get(m.group(1), "") + src[m.end():end]
    return out


def reached(funcs, name):
    """The HIP calls of `name`'s body and of the bodies of the file's functions it calls, transitively."""
    seen, todo, text = set(), [name], ""
    while todo:
        f = todo.pop()
        if f in seen:
            continue
        seen.add(f)
        text += funcs[f]
        todo += [g for g in funcs if g not in seen and re.search(r"\b%s\s*\(" % re.escape(g), funcs[f])]
    return set(re.findall(r"\bhip\w+", text))


def test_the_classes_are_what_engine_hip_does():
    funcs = engine_functions()
    for name, (cls, _) in list(CALLS.items()) + list(NO_STREAM.items()):
        assert name in funcs, name
        hip = reached(funcs, name)
        for call in REACHES[cls]:
            assert call in hip, (name, cls, call)
        for call in WAITS:
            if call not in REACHES[cls]:
                assert call not in hip, (name, cls, call)
    # no entry point outside the two tables waits for a stream or the device, but the create / destroy pair and the
    # diagnostic-build stamp readers
    others = {n for n in funcs if n.startswith("zs_")} - set(CALLS) - set(NO_STREAM)
    waiting = {n for n in others if reached(funcs, n) & set(WAITS)}
    assert waiting <= {"zs_create", "zs_destroy", "zs_debug_stamps", "zs_debug_stamps_wg", "zs_debug_timeline"}, waiting
