"""Launch-trace recorder: what a piece of code asks of ``segmantic_amd.ops`` and of the HIP stream ordering, in a form
two runs can be compared in.

``with record() as trace:`` wraps, for its duration, every function defined at module level in ``segmantic_amd.ops``,
``ops.WpackBatch.run``, ``torch.cuda.Stream.wait_event`` / ``wait_stream`` and ``torch.cuda.Event.record``, and appends
one event per call to ``trace.events``:

    ["ev", name, number of torch.cuda.current_stream(), arguments, returned value]

Arguments are bound to the callee's signature (defaults applied), so a positional and a keyword spelling of one call
are one event.  Canonical forms:

    tensor        ["T", storage number by first appearance, byte offset into it, shape, stride, dtype]
    WindowBatch   ["W", its volume as a tensor, starts, roi]
    tuple / list  ["L", element, ...]
    None, bool, int, str   as is
    float         ["F", repr]
    stream, event, WpackBatch   ["S" | "E" | "B", number by first appearance]
    torch.dtype   ["D", name]
    the returned value is kept for bool / int / str results, else None

The recorder keeps a reference to every storage (event, batch) it has numbered: no address is handed out twice within
a trace.  Two kinds of call leave no event: calls made from inside a recorded call (the callee's own helpers --
``Stream.wait_stream`` is built from ``Event.record`` + ``wait_event``), and calls none of whose arguments is a
tensor, window batch, stream, event or pack batch (``mfma_ok(cin, cout)``, ``wgrad_cus(n)``: host arithmetic on plain
numbers, touching neither memory nor a stream).

``encode`` / ``decode`` store traces with every descriptor and event interned in one table, so that a trace is a
list of integers.  The recorder knows nothing of the engine; what a trace must contain is the caller's business.
"""
from __future__ import annotations

import inspect
import json
import numbers
import types
from contextlib import contextmanager

import torch

from segmantic_amd import ops


class Trace:
    def __init__(self):
        self.events = []
        self._numbers = {"T": {}, "S": {}, "E": {}, "B": {}}
        self._keep = []
        self._depth = 0
        self._device_arg = False

    def _number(self, kind, key, obj):
        table = self._numbers[kind]
        if key not in table:
            table[key] = len(table)
            self._keep.append(obj)
        self._device_arg = True
        return table[key]

    def canon(self, v):
        if v is None or isinstance(v, (bool, int, str)):
            return v
        if isinstance(v, float):
            return ["F", repr(v)]
        if isinstance(v, numbers.Real):             # numpy scalars
            return int(v) if isinstance(v, numbers.Integral) else ["F", repr(float(v))]
        if isinstance(v, torch.Tensor):
            st = v.untyped_storage()
            no = self._number("T", st.data_ptr(), st)
            return ["T", no, v.data_ptr() - st.data_ptr(), list(v.shape), list(v.stride()), str(v.dtype)[6:]]
        if isinstance(v, ops.WindowBatch):
            return ["W", self.canon(v.volume), self.canon(v.starts), self.canon(v.roi)]
        if isinstance(v, (tuple, list)):
            return ["L"] + [self.canon(e) for e in v]
        if isinstance(v, torch.cuda.Stream):
            return ["S", self._number("S", v.cuda_stream, v)]
        if isinstance(v, torch.cuda.Event):
            return ["E", self._number("E", id(v), v)]
        if isinstance(v, ops.WpackBatch):
            return ["B", self._number("B", id(v), v)]
        if isinstance(v, torch.dtype):
            return ["D", str(v)[6:]]
        return ["O", type(v).__name__]

    def wrap(self, name, fn, bind=None):
        sig = inspect.signature(fn)

        def traced(*a, **k):
            if self._depth:
                return fn(*a, **k)
            bound = sig.bind(*a, **k)
            bound.apply_defaults()
            values = list(bound.arguments.values())
            if bind is not None:
                values = bind(*values)
            self._device_arg = False
            args = self.canon(values)
            recorded = self._device_arg
            stream = self.canon(torch.cuda.current_stream())[1]
            self._depth += 1
            try:
                ret = fn(*a, **k)
            finally:
                self._depth -= 1
            if recorded:
                self.events.append(["ev", name, stream, args, ret if isinstance(ret, (bool, int, str)) else None])
            return ret
        return traced


@contextmanager
def record():
    trace = Trace()
    targets = [(ops, n, n, None) for n, f in vars(ops).items()
               if isinstance(f, types.FunctionType) and f.__module__ == ops.__name__]
    targets += [(ops.WpackBatch, "run", "WpackBatch.run", None),
                (torch.cuda.Stream, "wait_event", "Stream.wait_event", None),
                (torch.cuda.Stream, "wait_stream", "Stream.wait_stream", None),
                # an event recorded without a stream goes to the current one
                (torch.cuda.Event, "record", "Event.record",
                 lambda ev, stream=None: [ev, stream if stream is not None else torch.cuda.current_stream()])]
    saved = []
    try:
        for obj, attr, name, bind in targets:
            orig = obj.__dict__[attr]
            saved.append((obj, attr, orig))
            setattr(obj, attr, trace.wrap(name, orig, bind))
        yield trace
    finally:
        for obj, attr, orig in reversed(saved):
            setattr(obj, attr, orig)


# ------------------------------------------------------------------------------------------------ storage
def encode(traces: dict) -> dict:
    """{config: events} -> {"table": [...], "traces": {config: [table index, ...]}}.  Scalars and leaf descriptors are
    table entries as they are; the elements of ["L" | "W", ...], the name, arguments and result of an event and the
    ["V", shape, stride, dtype] of a tensor are table indices."""
    table, index = [], {}

    def intern(v):
        if isinstance(v, list) and v[0] in ("L", "W"):
            v = v[:1] + [intern(e) for e in v[1:]]
        elif isinstance(v, list) and v[0] == "T":
            v = v[:3] + [intern(["V"] + v[3:])]
        elif isinstance(v, list) and v[0] == "ev":
            v = ["ev", intern(v[1]), v[2], intern(v[3]), intern(v[4])]
        key = json.dumps(v)
        if key not in index:
            index[key] = len(table)
            table.append(v)
        return index[key]

    return {"table": table, "traces": {name: [intern(ev) for ev in events] for name, events in traces.items()}}


def decode(stored: dict) -> dict:
    table = stored["table"]

    def expand(i):
        v = table[i]
        if isinstance(v, list) and v[0] in ("L", "W"):
            return v[:1] + [expand(e) for e in v[1:]]
        if isinstance(v, list) and v[0] == "T":
            return v[:3] + table[v[3]][1:]
        if isinstance(v, list) and v[0] == "ev":
            return ["ev", table[v[1]], v[2], expand(v[3]), expand(v[4])]
        return v

    return {name: [expand(i) for i in seq] for name, seq in stored["traces"].items()}


def dumps(stored: dict) -> str:
    """the golden file's text: one line per table entry and per trace"""
    rows = ",\n".join(json.dumps(v, separators=(",", ":")) for v in stored["table"])
    seqs = ",\n".join(f"{json.dumps(n)}:{json.dumps(s, separators=(',', ':'))}" for n, s in stored["traces"].items())
    return '{"table":[\n' + rows + '\n],\n"traces":{\n' + seqs + "\n}}\n"


def show(event) -> str:
    """an event as one readable line"""
    def txt(v):
        if not isinstance(v, list):
            return repr(v)
        if v[0] == "T":
            return f"T{v[1]}+{v[2]}{v[3]}/{v[4]}:{v[5]}"
        if v[0] == "L":
            return "(" + ", ".join(txt(e) for e in v[1:]) + ")"
        if v[0] == "W":
            return f"Windows({txt(v[1])}, starts={txt(v[2])}, roi={txt(v[3])})"
        return f"{v[0]}{v[1]}"
    _, name, stream, args, ret = event
    return f"[stream {stream}] {name}{txt(args)} -> {ret!r}"


def first_difference(got, want):
    """None when the two event lists are equal, else a message naming the first index at which they differ"""
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return f"event {i} differs\n  recorded: {show(w)}\n  now:      {show(g)}"
    if len(got) != len(want):
        i = min(len(got), len(want))
        extra = got[i] if len(got) > len(want) else want[i]
        return (f"{len(got)} events now, {len(want)} recorded; the {'new' if len(got) > len(want) else 'recorded'} "
                f"trace goes on with\n  {show(extra)}")
    return None
