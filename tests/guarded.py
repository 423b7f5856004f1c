"""Guard bands around the operands of one kernel call: what a kernel does AROUND its arrays.

Every operand lies in one flat array [guard | body | guard].  An input's guards hold a quiet NaN with a payload of
its own; an output's guards AND its body hold a second one ("poison").  After the call the flat arrays are read back
and compared, as unsigned words, with what went in:

  (a) a guard word of an output changed: a store in front of the array or behind its end;
  (b) a body word of an output is still poison: an element no launch wrote (an output that accumulates, `y += ...`,
      keeps the poison's NaN too, with or without its payload: (b) or (d));
  (c) a word of an input changed, body or guard;
  (d) an output holds a non-finite value: with finite inputs, something read from a NaN guard reached it;
  (e) an element that the header documents as left alone was written (`untouched`, stated by the case).

The numpy part (layout, verdict) knows nothing of a device and is held by tests/test_guarded_host.py on stand-ins
that commit each of these; the device part (Guarded) is one eng.to_device of the flat array and a
DeviceArray.from_pointer view of its body.  A read that strays and reaches no output is invisible here, by design."""

import collections
import contextlib

import numpy as np

IN_NAN, OUT_NAN = 0x7FC1A5A5, 0x7FC5EED5        # quiet NaNs with recognisable payloads: input guards; output poison
IN_BYTE, OUT_BYTE = 0xA5, 0x5A                  # ... of byte arrays
FLAT_GUARD = 1024                               # elements per side of a flat or byte array
KINDS = {'a': 'a guard word changed', 'b': 'still poison', 'c': 'an input changed', 'd': 'a non-finite value',
         'e': 'an element documented as untouched was written'}

Span = collections.namedtuple('Span', 'name role start size dtype untouched')
Finding = collections.namedtuple('Finding', 'kind name offset count')


def plane_guard(h, w):
    """Guard elements per side of an array of h x w planes: a surplus channel's first row, or a surplus patch row,
    lands in the guard at any patch position.  (The rear guard has exactly this many; the front one is rounded up
    to whole 16 bytes, plus a case's offset: lead().)"""
    return int(h) * int(w) + FLAT_GUARD


def default_guard(shape):
    return plane_guard(shape[-2], shape[-1]) if len(shape) == 3 else FLAT_GUARD


def _words(dtype):
    """The unsigned type an array of `dtype` is compared as."""
    return {1: np.uint8, 4: np.uint32}[np.dtype(dtype).itemsize]


def pattern(dtype, role):
    wide = np.dtype(dtype).itemsize == 4
    if role == 'input':
        return _words(dtype)(IN_NAN if wide else IN_BYTE)
    return _words(dtype)(OUT_NAN if wide else OUT_BYTE)


def lead(guard, dtype, offset=0):
    """Elements in front of the body: at least `guard`, the body 16-byte aligned, then `offset` bytes (0, 4 or 8) on."""
    item = np.dtype(dtype).itemsize
    assert offset % item == 0 and 0 <= offset < 16
    per16 = 16 // item
    return -(-int(guard) // per16) * per16 + offset // item


def layout(host, guard, fill, offset=0):
    """One flat array [guard | body | guard] of host's dtype.  fill 'input': the body is host, the guards the input
    pattern; fill 'output': guards and body are poison (host gives shape and dtype only).  The body starts at
    lead(guard, dtype, offset) and the flat array's own start is taken as 16-byte aligned."""
    host = np.asarray(host)
    assert fill in ('input', 'output')
    start = lead(guard, host.dtype, offset)
    flat = np.full(start + host.size + int(guard), pattern(host.dtype, fill), _words(host.dtype))
    if fill == 'input':
        flat[start:start + host.size] = np.ascontiguousarray(host).reshape(-1).view(_words(host.dtype))
    return flat.view(host.dtype)


def span_of(name, host, guard, fill, offset=0, untouched=None):
    host = np.asarray(host)
    if untouched is not None:
        untouched = np.ascontiguousarray(np.broadcast_to(untouched, host.shape)).reshape(-1).astype(bool)
    return Span(name, fill, lead(guard, host.dtype, offset), host.size, host.dtype, untouched)


def _first(mask):
    hits = np.flatnonzero(mask)
    return (int(hits[0]), int(hits.size)) if hits.size else None


def verdict(before, after, spans):
    """Findings of one call: before / after {name: flat array}, spans the operands.  Each finding names the operand,
    the first offending offset RELATIVE TO THE BODY (negative: the front guard; >= size: the rear one) and how many
    words offend; [] is a clean call."""
    found = []

    def add(kind, span, mask, base):
        hit = _first(mask)
        if hit:
            found.append(Finding(kind, span.name, hit[0] + base, hit[1]))

    for sp in spans:
        w = _words(sp.dtype)
        b, a = np.asarray(before[sp.name]).view(w), np.asarray(after[sp.name]).view(w)
        assert b.shape == a.shape, sp.name
        end = sp.start + sp.size
        changed = a != b
        if sp.role == 'input':
            add('c', sp, changed, -sp.start)
            continue
        add('a', sp, changed[:sp.start], -sp.start)
        add('a', sp, changed[end:], sp.size)
        body = a[sp.start:end]
        poison = body == pattern(sp.dtype, 'output')
        keep = sp.untouched if sp.untouched is not None else np.zeros(sp.size, bool)
        add('b', sp, poison & ~keep, 0)
        add('e', sp, ~poison & keep, 0)
        if np.dtype(sp.dtype).kind == 'f':
            add('d', sp, ~np.isfinite(body.view(sp.dtype)) & ~poison, 0)
    return found


def describe(found):
    return '\n'.join('  (%s) %s: %s at offset %d of the body, %d word(s)' % (f.kind, f.name, KINDS[f.kind], f.offset, f.count)
                     for f in found)


class HostGuarded:
    """The bookkeeping of one guarded call on numpy arrays (the stand-ins of tests/test_guarded_host.py run on
    these; Guarded below puts the same flat arrays on a device)."""

    def __init__(self):
        self.spans, self.flat, self.before = [], {}, {}

    def _add(self, name, host, guard, fill, offset, untouched=None):
        assert name not in self.flat, name
        host = np.asarray(host)
        guard = default_guard(host.shape) if guard is None else guard
        sp = span_of(name, host, guard, fill, offset, untouched)
        self.spans.append(sp)
        self.flat[name] = layout(host, guard, fill, offset)
        self.before[name] = self.flat[name].copy()
        return sp

    def input(self, name, host, guard=None, offset=0):
        """-> the flat array and the span; the body is flat[span.start:span.start + span.size]."""
        sp = self._add(name, host, guard, 'input', offset)
        return self.flat[name], sp

    def output(self, name, shape, dtype=np.float32, guard=None, offset=0, untouched=None):
        sp = self._add(name, np.empty(shape, dtype), guard, 'output', offset, untouched)
        return self.flat[name], sp

    def findings(self):
        return verdict(self.before, self.flat, self.spans)


class Guarded:
    """One hook call under guard bands on an engine's device.  input() / output() return a DeviceArray view of the
    body; check() reads everything back, leaves the outputs' bodies in .out and returns the findings; free() gives
    the device memory back."""

    def __init__(self, eng):
        self.eng, self.host = eng, HostGuarded()
        self.dev, self.shapes, self.out = {}, {}, {}

    def _view(self, name, sp, shape):
        from style_transfer_amd.engine import DeviceArray
        flat = self.host.flat[name]
        owner = self.eng.to_device(flat.view(_words(sp.dtype)), _words(sp.dtype))
        assert owner.ptr % 16 == 0
        self.dev[name], self.shapes[name] = owner, tuple(shape)
        item = np.dtype(sp.dtype).itemsize
        return DeviceArray.from_pointer(self.eng, owner.ptr + sp.start * item, shape, sp.dtype, owner=owner)

    def input(self, name, host, guard=None, offset=0, dtype=np.float32):
        host = np.ascontiguousarray(host, dtype)
        _, sp = self.host.input(name, host, guard, offset)
        return self._view(name, sp, host.shape)

    def output(self, name, shape, dtype=np.float32, guard=None, offset=0, untouched=None):
        _, sp = self.host.output(name, shape, dtype, guard, offset, untouched)
        return self._view(name, sp, shape)

    def check(self):
        after = {}
        for sp in self.host.spans:
            flat = self.dev[sp.name].get().view(sp.dtype)
            after[sp.name] = flat
            if sp.role == 'output':
                self.out[sp.name] = flat[sp.start:sp.start + sp.size].reshape(self.shapes[sp.name]).copy()
        return verdict(self.host.before, after, self.host.spans)

    def free(self):
        for arr in self.dev.values():
            arr.free()
        self.dev = {}


@contextlib.contextmanager
def guarded_call(eng, what=''):
    """with guarded_call(eng) as g: build the operands with g.input / g.output and make ONE hook call.  On the way
    out everything is read back (g.out[name]: the outputs' bodies) and the verdict must be empty; all findings are
    printed otherwise."""
    g = Guarded(eng)
    try:
        yield g
        found = g.check()
        assert not found, '%s: the call left its arrays\n%s' % (what, describe(found))
    finally:
        g.free()
