"""A small numpy evaluator for the vector instructions the translator emits into the body of a steady fast or quiet stream
(fx_xlate.cpp), driven by the assembler listing of FrontEnd.translate: test_xlate_emitted.py runs the emitted code itself on the
CPU, not a model of the records.

Registers are uint32 columns, one element per case; vcc is a boolean column; SGPRs are plain words (uniform).  fp32 arithmetic
goes through np.float32 (round to nearest even, denormals kept - the mode of every generated stream), the fused operations
(v_fma_f32, v_fma_f64) and the fp64 ones through exact integer arithmetic with ONE rounding.  Source modifiers (|v|, -v), inline
constants and 32-bit literals are read as the listing prints them.  Scalar, branch, wait and memory instructions are passed over
(`s_mov_b32 sN, literal` is kept: vector instructions read such SGPRs) - but a vector mnemonic the evaluator does not know is
refused by name, never passed over."""
import math
import re

import numpy as np

INLINE_F = {"0.5": 0.5, "-0.5": -0.5, "1.0": 1.0, "-1.0": -1.0, "2.0": 2.0, "-2.0": -2.0, "4.0": 4.0, "-4.0": -4.0}
SKIPPED = ("s_", "global_", "buffer_", "flat_", "scratch_", "ds_")


class UnknownMnemonic(Exception):
    pass


def _split(x):
    """a finite double as (m, e): x == m * 2**e with an integer m"""
    m, e = math.frexp(x)
    return int(m * (1 << 53)), e - 53


def _rounded(total, e, precision, min_ulp):
    """total * 2**e (total an integer, not 0) rounded to nearest even with `precision` significant bits and no ulp below
    2**min_ulp: as a double (exact for fp32 results too)"""
    a = abs(total)
    ulp = max(e + a.bit_length() - precision, min_ulp)
    shift = ulp - e
    if shift <= 0:
        q = a << -shift
    else:
        q, rem, half = a >> shift, a & ((1 << shift) - 1), 1 << (shift - 1)
        if rem > half or (rem == half and q & 1):
            q += 1
    return math.copysign(math.ldexp(q, ulp), total)


def fma_exact(a, b, c, precision, min_ulp):
    """a * b + c of finite doubles with one rounding to the given format"""
    (ma, ea), (mb, eb), (mc, ec) = _split(a), _split(b), _split(c)
    p, ep = ma * mb, ea + eb
    if p == 0 and mc == 0:
        sp = math.copysign(1.0, a) * math.copysign(1.0, b)
        return c if math.copysign(1.0, c) == sp else 0.0          # (+-0) + (-+0) is +0 under round to nearest
    if p == 0:
        return _rounded(mc, ec, precision, min_ulp)
    if mc == 0:
        return _rounded(p, ep, precision, min_ulp)
    e = min(ep, ec)
    total = (p << (ep - e)) + (mc << (ec - e))
    return 0.0 if total == 0 else _rounded(total, e, precision, min_ulp)   # an exact cancellation gives +0


F32 = (24, -149)
F64 = (53, -1074)


class Valu:
    def __init__(self, cases):
        self.cases = cases
        self.v = {}          # VGPR number -> uint32 column
        self.s = {}          # SGPR number -> word
        self.vcc = None
        self.executed = {}   # mnemonic -> count
        self.loaded = []     # VGPRs a passed-over load writes, in order

    # ---- operands
    def _word(self, n, what):
        if n not in self.v:
            raise KeyError("%s reads v%d, which nothing has written" % (what, n))
        return self.v[n]

    def f32(self, text, what):
        """a source as a float32 column"""
        neg = text.startswith("-") and not re.match(r"-\d", text)
        if neg:
            text = text[1:]
        mag = text.startswith("|") and text.endswith("|")
        if mag:
            text = text[1:-1]
        m = re.match(r"v(\d+)$", text)
        if m:
            col = self._word(int(m.group(1)), what).view(np.float32)
        else:
            col = np.full(self.cases, self.bits(text, what), dtype=np.uint32).view(np.float32)
        if mag:
            col = np.abs(col)
        return -col if neg else col

    def bits(self, text, what):
        """a uniform source's word: SGPR, 32-bit literal, inline float or inline integer"""
        m = re.match(r"s(\d+)$", text)
        if m:
            if int(m.group(1)) not in self.s:
                raise KeyError("%s reads s%s, which no s_mov_b32 of the listing has set" % (what, m.group(1)))
            return self.s[int(m.group(1))]
        if text in INLINE_F:
            return int(np.float32(INLINE_F[text]).view(np.uint32))
        if re.match(r"0x[0-9a-f]+$", text):
            return int(text, 16)
        if re.match(r"-?\d+$", text) and -16 <= int(text) <= 64:
            return int(text) & 0xffffffff
        raise ValueError("%s: operand %r" % (what, text))

    def raw(self, text, what):
        m = re.match(r"v(\d+)$", text)
        return self._word(int(m.group(1)), what) if m else np.full(self.cases, self.bits(text, what), dtype=np.uint32)

    def f64(self, text, what):
        """a 64-bit source as a list of doubles"""
        m = re.match(r"v\[(\d+):(\d+)\]$", text)
        if m:
            lo, hi = self._word(int(m.group(1)), what), self._word(int(m.group(2)), what)
            return (lo.astype(np.uint64) | (hi.astype(np.uint64) << np.uint64(32))).view(np.float64).tolist()
        m = re.match(r"s\[(\d+):(\d+)\]$", text)
        if m:
            w = self.bits("s" + m.group(1), what) | (self.bits("s" + m.group(2), what) << 32)
            return [float(np.array([w], dtype=np.uint64).view(np.float64)[0])] * self.cases
        if text in INLINE_F:
            return [INLINE_F[text]] * self.cases
        if text == "0":
            return [0.0] * self.cases
        raise ValueError("%s: 64-bit operand %r" % (what, text))

    def put(self, text, col):
        self.v[int(re.match(r"v(\d+)$", text).group(1))] = np.ascontiguousarray(col, dtype=np.float32).view(np.uint32).copy()

    def put64(self, text, doubles):
        m = re.match(r"v\[(\d+):(\d+)\]$", text)
        w = np.array(doubles, dtype=np.float64).view(np.uint64)
        self.v[int(m.group(1))] = (w & np.uint64(0xffffffff)).astype(np.uint32)
        self.v[int(m.group(2))] = (w >> np.uint64(32)).astype(np.uint32)

    # ---- one instruction
    def step(self, line):
        line = line.strip()
        if not line or line.startswith(";"):
            return
        op, _, rest = line.partition(" ")
        a = [t.strip() for t in rest.split(",")] if rest else []
        if op == "s_mov_b32" and re.match(r"s\d+$", a[0]) and not re.match(r"[sv]|exec|vcc|m0", a[1]):
            self.s[int(a[0][1:])] = self.bits(a[1], line)
            return
        if op.startswith(SKIPPED):
            if op.startswith("global_load"):
                self.loaded.append(int(re.match(r"v(\d+)$", a[0]).group(1)))
            return
        if not op.startswith("v_"):
            raise UnknownMnemonic(op)
        with np.errstate(all="ignore"):
            self._vector(op, a, line)
        self.executed[op] = self.executed.get(op, 0) + 1

    def _vector(self, op, a, line):
        f = lambda k: self.f32(a[k], line)   # noqa: E731
        if op == "v_mul_f32_e32":
            self.put(a[0], f(1) * f(2))
        elif op == "v_add_f32_e32":
            self.put(a[0], f(1) + f(2))
        elif op == "v_sub_f32_e32":
            self.put(a[0], f(1) - f(2))
        elif op == "v_subrev_f32_e32":
            self.put(a[0], f(2) - f(1))
        elif op == "v_med3_f32":
            x, y, z = f(1), f(2), f(3)
            assert np.isfinite(x).all() and np.isfinite(y).all() and np.isfinite(z).all(), line
            self.put(a[0], np.maximum(np.minimum(x, y), np.minimum(np.maximum(x, y), z)))
        elif op == "v_max3_f32":
            self.put(a[0], np.maximum(np.maximum(f(1), f(2)), f(3)))
        elif op == "v_fma_f32":
            x, y, z = (c.astype(np.float64).tolist() for c in (f(1), f(2), f(3)))
            self.put(a[0], np.array([fma_exact(p, q, r, *F32) for p, q, r in zip(x, y, z)], dtype=np.float64).astype(np.float32))
        elif op == "v_mov_b32_e32":
            self.v[int(a[0][1:])] = self.raw(a[1], line).copy()
        elif op == "v_cvt_f64_f32_e32":
            self.put64(a[0], f(1).astype(np.float64))
        elif op == "v_cvt_f32_f64_e32":
            self.put(a[0], np.array(self.f64(a[1], line), dtype=np.float64).astype(np.float32))
        elif op == "v_fma_f64":
            x, y, z = (self.f64(a[k], line) for k in (1, 2, 3))
            self.put64(a[0], [fma_exact(p, q, r, *F64) for p, q, r in zip(x, y, z)])
        elif op == "v_mul_f64":
            x, y = self.f64(a[1], line), self.f64(a[2], line)
            self.put64(a[0], [fma_exact(p, q, math.copysign(0.0, p) * math.copysign(1.0, q), *F64) for p, q in zip(x, y)])
        elif op == "v_add_f64":
            x, y = self.f64(a[1], line), self.f64(a[2], line)
            self.put64(a[0], [fma_exact(p, 1.0, q, *F64) for p, q in zip(x, y)])
        elif op == "v_cndmask_b32_e32":
            assert a[3] == "vcc" and self.vcc is not None, line
            self.v[int(a[0][1:])] = np.where(self.vcc, self.raw(a[2], line), self.raw(a[1], line)).astype(np.uint32)
        elif op == "v_cmp_lt_f32_e32":
            assert a[0] == "vcc", line
            self.vcc = f(1) < f(2)
        elif op == "v_cmp_ge_f32_e32":
            assert a[0] == "vcc", line
            self.vcc = f(1) >= f(2)
        else:
            raise UnknownMnemonic(op)

    def run(self, lines):
        for l in lines:
            self.step(l)
        return self
