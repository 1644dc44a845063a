"""Plain-Python restatement of how the reference evaluates a predicate over data rows, written from the
Java (kernel-defaults/src/main/java/io/delta/kernel/defaults/internal/expressions/):

  * DefaultPredicateEvaluator.java:42-72 -- the predicate is ANDed with `existing selection = true`; a row
    is kept iff that AND is TRUE (null and false both drop the row);
  * DefaultExpressionEvaluator.java:384-437 -- AND / OR in Kleene logic, both children always evaluated;
    :554-561 NOT (null stays null); :563-575 IS_NOT_NULL / IS_NULL (never null); :440-447 ALWAYS_TRUE /
    ALWAYS_FALSE; :450-468 the comparators, over children cast to a common type first (:337-354,
    ImplicitCastExpression.java:30-41: byte < short < integer < long < float < double);
  * DefaultExpressionUtils.java:64-75 evalNullability -- a comparison with a null operand is null (:182-216),
    except IS NOT DISTINCT FROM (:224-269: two nulls are equal, one null is unequal);
  * DefaultExpressionUtils.java:119-173 getComparator -- Boolean / Byte / Short / Integer / Long.compare,
    Float.compare / Double.compare (NaN greatest and equal to itself, -0.0 < 0.0), BigDecimal natural
    order (by value, any scale), strings by their UTF-8 bytes (:51-56) and binary (:40-50) as unsigned
    bytes, then by length.

Rows are dicts {column path tuple: value}; values are None, bool, int (integral types, date days,
timestamp micros), float (float / double; a float column's values are binary32 values), str, bytes or
decimal.Decimal. `types` maps a column path to its Kernel type name."""
import math
import struct
from decimal import Decimal

from delta_amd.expressions import Column, Literal, Predicate

_ORDER = ["byte", "short", "integer", "long", "float", "double"]


def java_fp_compare(a: float, b: float) -> int:
    """Float.compare / Double.compare."""
    an, bn = math.isnan(a), math.isnan(b)
    if an or bn:
        return int(an) - int(bn)
    if a < b:
        return -1
    if a > b:
        return 1
    sa, sb = math.copysign(1.0, a) < 0, math.copysign(1.0, b) < 0
    return 0 if sa == sb else (-1 if sa else 1)


def _f32(x) -> float:
    """(float) x: round to binary32 (Java's long -> float and double -> float conversions)."""
    try:
        return struct.unpack("<f", struct.pack("<f", float(x)))[0]
    except OverflowError:
        return math.copysign(math.inf, x)


def _type_of(e, types):
    if isinstance(e, Column):
        return types[tuple(e.names)]
    if isinstance(e, Literal):
        return e.type
    return "boolean"


def _value(e, row, types):
    if isinstance(e, Column):
        return row.get(tuple(e.names))
    if isinstance(e, Literal):
        return e.value
    return evaluate(e, row, types)


def _compare(a, ta, b, tb) -> int:
    if ta in _ORDER and tb in _ORDER:
        wide = _ORDER[max(_ORDER.index(ta), _ORDER.index(tb))]
        if wide == "float":
            return java_fp_compare(_f32(a), _f32(b))
        if wide == "double":
            return java_fp_compare(float(a), float(b))
        return (a > b) - (a < b)
    if ta != tb and not (ta.startswith("decimal") and tb.startswith("decimal")):
        raise TypeError("operands of different types: %s, %s" % (ta, tb))
    if ta == "string":
        a, b = a.encode("utf-8"), b.encode("utf-8")     # STRING_COMPARATOR: UTF-8 bytes
    if ta in ("string", "binary"):
        a, b = bytes(a), bytes(b)                       # unsigned bytes, then length
    if ta.startswith("decimal"):
        a, b = Decimal(a), Decimal(b)
    return (a > b) - (a < b)


def evaluate(p, row, types):
    """True / False / None (SQL null)."""
    if isinstance(p, Literal):
        return p.value
    if isinstance(p, Column):
        return row.get(tuple(p.names))
    n, c = p.name.upper(), p.children
    if n == "ALWAYS_TRUE":
        return True
    if n == "ALWAYS_FALSE":
        return False
    if n in ("AND", "OR"):
        l, r = evaluate(c[0], row, types), evaluate(c[1], row, types)     # both sides, always
        if n == "AND":
            return False if (l is False or r is False) else True if (l is True and r is True) else None
        return True if (l is True or r is True) else False if (l is False and r is False) else None
    if n == "NOT":
        v = evaluate(c[0], row, types)
        return None if v is None else not v
    if n in ("IS_NULL", "IS_NOT_NULL"):
        v = _value(c[0], row, types)
        return (v is None) == (n == "IS_NULL")
    a, b = _value(c[0], row, types), _value(c[1], row, types)
    if n == "IS NOT DISTINCT FROM":
        if a is None or b is None:
            return a is None and b is None
        return _compare(a, _type_of(c[0], types), b, _type_of(c[1], types)) == 0
    if a is None or b is None:
        return None
    k = _compare(a, _type_of(c[0], types), b, _type_of(c[1], types))
    return {"<": k < 0, "<=": k <= 0, ">": k > 0, ">=": k >= 0, "=": k == 0}[n]


def keep(p, row, types, existing=True) -> bool:
    """DefaultPredicateEvaluator: AND(existing = true, predicate) is TRUE."""
    return bool(existing) and (p is None or evaluate(p, row, types) is True)
