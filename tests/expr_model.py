"""An independent model of the expression semantics (include/ytql_gpu.h, the
comment above YtExpr), in plain Python. It shares no code with the C
evaluators (eval_prog, heval, the oracle's eval_expr) nor with api.py's
helpers: the tests hold all three against it.

Trees are tuples:
    ("col", i)  ("lit", n)  ("litf", x)  ("null",)  ("not", a)  (op, a, b)
with op one of ARITH, REL or "and" / "or". Values are (type, value) pairs
with None for null. An INT64 value is a Python int in [-2**63, 2**63), a
UINT64 value one in [0, 2**64), a BOOLEAN value the raw 64-bit pattern as an
unsigned int (a comparison yields 0 or 1; arithmetic over booleans is unsigned
64-bit arithmetic over those patterns), a DOUBLE value a Python float.
"""
import math
import struct

I64, U64, DBL, BOOL, NUL = "int64", "uint64", "double", "boolean", "null"

ARITH = ("+", "-", "*", "//", "%")
REL = ("==", "!=", "<", "<=", ">", ">=")

STACK_SLOTS = 12        # evaluation stack of the device interpreter
MAX_PROGRAM = 48        # instructions over all programs of one plan

M64 = (1 << 64) - 1


class Refused(Exception):
    """a static verdict: the plan is refused before it runs"""

    def __init__(self, verdict):
        Exception.__init__(self, verdict)
        self.verdict = verdict


class DivZero(Exception):
    """an integer division or modulo met a zero divisor on some row"""


def dbl_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def bits_of(v):
    """the 64-bit pattern of a non-null value"""
    t, x = v
    if t == DBL:
        return dbl_bits(x)
    return x & M64


def _from_bits(t, z):
    z &= M64
    if t == I64:
        return (t, z - (1 << 64) if z >> 63 else z)
    return (t, z)


# ---- static typing -------------------------------------------------------

def _adopt(e, own, other):
    """the type operand e has beside an operand of static type `other`"""
    if e[0] != "lit":
        return own
    if other == DBL:
        return DBL
    if other == U64:
        if e[1] < 0:
            raise Refused("type mismatch")
        return U64
    return own


def _operand_types(e, col_types):
    ta = static_type(e[1], col_types)
    tb = static_type(e[2], col_types)
    xa = _adopt(e[1], ta, tb)
    xb = _adopt(e[2], tb, ta)
    if (xa == DBL and xb not in (DBL, NUL)) or (xb == DBL and xa not in (DBL, NUL)):
        raise Refused("type mismatch")
    if {xa, xb} == {I64, U64}:
        raise Refused("type mismatch")
    return xa, xb


def static_type(e, col_types):
    """the static type of e; raises Refused("type mismatch") or
    Refused("unsupported") (modulo over doubles)"""
    k = e[0]
    if k == "col":
        return col_types[e[1]]
    if k == "lit":
        return I64
    if k == "litf":
        return DBL
    if k == "null":
        return NUL
    if k == "not":
        static_type(e[1], col_types)
        return BOOL
    if k in ("and", "or"):
        static_type(e[1], col_types)
        static_type(e[2], col_types)
        return BOOL
    xa, xb = _operand_types(e, col_types)
    if k in REL:
        return BOOL
    assert k in ARITH, k
    t = xb if xa == NUL else xa
    if k == "%" and t == DBL:
        raise Refused("unsupported")
    return t


def stack_need(e):
    k = e[0]
    if k in ("col", "lit", "litf", "null"):
        return 1
    if k == "not":
        return stack_need(e[1])
    return max(stack_need(e[1]), 1 + stack_need(e[2]))


def program_len(e):
    k = e[0]
    if k in ("col", "lit", "litf", "null"):
        return 1
    if k == "not":
        return 1 + program_len(e[1])
    return 1 + program_len(e[1]) + program_len(e[2])


def verdict(exprs, col_types):
    """"ok", or why a plan holding these expressions is refused: "type
    mismatch", "unsupported", "too deep" (one expression needs more than
    STACK_SLOTS) or "too long" (together more than MAX_PROGRAM instructions).
    Typing is judged first, as the entries do."""
    try:
        for e in exprs:
            static_type(e, col_types)
    except Refused as r:
        return r.verdict
    if any(stack_need(e) > STACK_SLOTS for e in exprs):
        return "too deep"
    if sum(program_len(e) for e in exprs) > MAX_PROGRAM:
        return "too long"
    return "ok"


# ---- evaluation ----------------------------------------------------------

def _operand(e, other_type, col_types, row):
    """the value of operand e beside an operand of static type other_type"""
    if e[0] == "lit":
        t = _adopt(e, I64, other_type)
        if t == DBL:
            return (DBL, float(e[1]))
        return (t, e[1])
    return evaluate(e, col_types, row)


def _truth(v):
    return bits_of(v) != 0


def _arith(op, t, a, b):
    if t == DBL:
        x, y = a[1], b[1]
        if op == "+":
            return (DBL, x + y)
        if op == "-":
            return (DBL, x - y)
        if op == "*":
            # inf * 0 and the like are NaN in IEEE; Python agrees
            return (DBL, x * y)
        if op == "//":
            return (DBL, _fdiv(x, y))
        raise Refused("unsupported")
    x, y = bits_of(a), bits_of(b)
    if op == "+":
        return _from_bits(t, x + y)
    if op == "-":
        return _from_bits(t, x - y)
    if op == "*":
        return _from_bits(t, x * y)
    if y == 0:
        raise DivZero()
    if t == I64:
        sx, sy = _from_bits(I64, x)[1], _from_bits(I64, y)[1]
        q = abs(sx) // abs(sy)
        if (sx < 0) != (sy < 0):
            q = -q                       # truncation toward zero
        r = sx - q * sy                  # takes the dividend's sign
        # INT64_MIN / -1 wraps to INT64_MIN, INT64_MIN % -1 is 0
        return _from_bits(I64, q if op == "//" else r)
    return _from_bits(t, x // y if op == "//" else x % y)


def _fdiv(x, y):
    """IEEE 754 division (Python raises on a zero divisor)"""
    if y == 0.0 and not math.isnan(x):
        if x == 0.0:
            return math.nan
        return math.copysign(math.inf, x) * math.copysign(1.0, y)
    return x / y if y != 0.0 else math.nan


def _compare(op, t, a, b):
    an, bn = a is None, b is None
    if an or bn:
        # null sorts below every value and equals null
        lt, eq = (an and not bn), (an == bn)
    elif t == DBL:
        if math.isnan(a[1]) or math.isnan(b[1]):
            return (BOOL, 1)             # unordered: all six are true
        lt, eq = a[1] < b[1], a[1] == b[1]
    elif t == I64:
        x, y = _from_bits(I64, bits_of(a))[1], _from_bits(I64, bits_of(b))[1]
        lt, eq = x < y, x == y
    else:
        x, y = bits_of(a), bits_of(b)
        lt, eq = x < y, x == y
    r = {"==": eq, "!=": not eq, "<": lt, "<=": lt or eq,
         ">": not (lt or eq), ">=": not lt}[op]
    return (BOOL, int(r))


def evaluate(e, col_types, row):
    """the value of e on one row (a list of (type, value) or None); the plan
    holding e has passed verdict(). Raises DivZero."""
    k = e[0]
    if k == "col":
        return row[e[1]]
    if k == "lit":
        return (I64, e[1])
    if k == "litf":
        return (DBL, e[1])
    if k == "null":
        return None
    if k == "not":
        a = evaluate(e[1], col_types, row)
        return None if a is None else (BOOL, int(not _truth(a)))
    if k in ("and", "or"):
        # Kleene; both operands are evaluated
        a = evaluate(e[1], col_types, row)
        b = evaluate(e[2], col_types, row)
        ta = None if a is None else _truth(a)
        tb = None if b is None else _truth(b)
        if k == "and":
            if ta is False or tb is False:
                return (BOOL, 0)
            return None if (ta is None or tb is None) else (BOOL, 1)
        if ta is True or tb is True:
            return (BOOL, 1)
        return None if (ta is None or tb is None) else (BOOL, 0)
    xa, xb = _operand_types(e, col_types)
    a = _operand(e[1], static_type(e[2], col_types), col_types, row)
    b = _operand(e[2], static_type(e[1], col_types), col_types, row)
    # the left operand's type decides how both patterns are read; a left
    # operand of static type null is null on every row
    t = xb if xa == NUL else xa
    if k in REL:
        return _compare(k, t, a, b)
    if a is None or b is None:
        return None                      # before any divisor is looked at
    return _arith(k, t, a, b)


def passes(v):
    """a filter's or HAVING's truth value: non-null and non-zero"""
    return v is not None and _truth(v)


def same(x, y):
    """value equality as the tests mean it: equal types; integers and
    booleans equal; doubles equal in every bit, except that any two NaNs
    count as equal"""
    if x is None or y is None:
        return x is None and y is None
    if x[0] != y[0]:
        return False
    if x[0] == DBL:
        if math.isnan(x[1]) and math.isnan(y[1]):
            return True
        return dbl_bits(x[1]) == dbl_bits(y[1])
    return bits_of(x) == bits_of(y)
