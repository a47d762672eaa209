"""The text of the reference's high-level vector columns, restated: SToJSON (SqliteSampleDescriptorPool.cpp:316-419) around
ToString(double, "%.9g") (Str.cpp:4027-4070).  A list is "[a,b,c]", a list of rows "[[a,b],[c,d]]", "," alone between the
numbers, an empty list "[]"; a number is what snprintf("%.9g") writes in the C locale -- Python's '%.9g' % v is the same
correctly rounded conversion -- and the values that are no numbers are spelled "NaN", "INF" and "-INF" (TStringConsts,
Str.cpp:719-721).  ToString's shortcut to "0.0" / "1.0" / "0.5" fires for the format "%.17lg" only, not for this one.

tests/test_text_format_cpu.py holds the restatement against KNOWN (glibc's answers) and against a C program that calls
snprintf; tests/test_gpu_high_level_text.py holds the GPU's text against it."""
import math

# glibc's snprintf("%.9g"): ties to even on exact halves, the switch to the exponent form, both ends of the doubles
KNOWN = [
    (100000000.5, "100000000"), (100000001.5, "100000002"), (12345678.25, "12345678.2"), (12345678.75, "12345678.8"),
    (1000000005.0, "1e+09"), (1000000015.0, "1.00000002e+09"), (999999999.5, "1e+09"), (99999999.95, "100000000"),
    (9.9999999995e-05, "0.0001"), (1e-05, "1e-05"), (123456789.0, "123456789"), (1234567890.0, "1.23456789e+09"),
    (4.9406564584124654e-324, "4.94065646e-324"), (1.7976931348623157e308, "1.79769313e+308"), (-0.0, "-0"), (0.1, "0.1"),
]
SPECIAL = [(math.nan, "NaN"), (-math.nan, "NaN"), (math.inf, "INF"), (-math.inf, "-INF")]


def g9(v):
    """one double as ToString(v, "%.9g") writes it"""
    v = float(v)
    if v != v:
        return "NaN"
    if v in (math.inf, -math.inf):
        return "INF" if v > 0 else "-INF"
    return "%.9g" % v


def json_list(values):
    """SToJSON of a TList<double>"""
    return "[" + ",".join(g9(v) for v in values) + "]"


def json_rows(rows):
    """SToJSON of a TList<TStaticArray<double, W>>: rows [n][W]"""
    return "[" + ",".join(json_list(r) for r in rows) + "]"


def json_column(a):
    """a 1-D array as a list, a 2-D array as a list of rows -> bytes"""
    return (json_rows(a) if getattr(a, "ndim", 1) == 2 else json_list(a)).encode("ascii")


def self_test():
    for v, want in KNOWN + SPECIAL:
        assert g9(v) == want, (v, g9(v), want)
    assert json_list([]) == "[]" and json_rows([]) == "[]"
    assert json_list([1.0, -0.0, 0.5]) == "[1,-0,0.5]"
    assert json_rows([[1.0, 2.5], [1e9, math.nan]]) == "[[1,2.5],[1e+09,NaN]]"


if __name__ == "__main__":
    self_test()
    print("tests/_json_ref.py: ok")
