"""Plain-Python restatement of what the reference makes of a file's class signature (AnalyzeHighLevelDescriptors,
SampleAnalyser.cpp:1097-1231), written from the reference's text, with serial sums in the reference's order:

* TClassificationTools::CategoryStrengths (ClassificationTools.cpp:7-39) and PickAllStrongCategories (:46-128), on indices:
  the caller holds the names and passes the index of the "None" class, or -1;
* TClassificationHeuristics::IsOneShot (ClassificationHeuristics.cpp:12-98) and IsLoop (:102-149), with
  TStatistics::Correlation (Statistics.cpp:604-638; MEpsilon = 1e-12f) and TAudioMath::DbToLin (AudioMath.inl:108-123);
* the override of the two class strengths (SampleAnalyser.cpp:1121-1148; MUseClassificationHeuristics is defined, :72) and
  the categories' gate (:1176-1231).

std::min, std::max and MMin (InlineMath.inl:22-25) are the comparisons they compile to, so that a NaN leaves the operand the
reference leaves.

PARITY UNPINNED: SampleAnalyser.cpp does not build here, so nothing in this file is held against the reference's objects."""
import math

import numpy as np

MIN_DEFAULT_WEIGHT, MIN_FALLBACK_WEIGHT = 0.2, 0.01                 # SA:1156-1157, :1211-1212
SILENCE_FLOOR = math.exp(-24.0 * (math.log(10.0) / 20.0))          # DbToLin(-24.0), ClassificationHeuristics.cpp:49
EPSILON = float(np.float32(1e-12))                                  # MEpsilon: a float literal widened to double
IS_ONESHOT, IS_LOOP, OVERRIDDEN = 1, 2, 4                           # the flags of afx_decision_out
SCALARS = ("effectve_length_24dB", "rhythm_percussive_onset_count", "rhythm_percussive_tempo_confidence",
           "rhythm_complex_tempo_confidence", "spectral_flux_mean")


def std_min(a, b):
    return b if b < a else a


def std_max(a, b):
    return b if a < b else a


def m_min(a, b):
    return a if a < b else b


def category_strengths(weights, min_weight=0.0):
    """ClassificationTools.cpp:7-39; the weights are the float signature widened to double (SA:1097)"""
    w = [float(v) for v in weights]
    total = 0.0
    for v in w:                                   # :16-22
        if v >= min_weight:
            total += v
    return [v / total if v >= min_weight and total > 0.0 else 0.0 for v in w]   # :24-36


def pick_all_strong(strengths, none=-1, min_default=MIN_DEFAULT_WEIGHT, min_fallback=MIN_FALLBACK_WEIGHT):
    """ClassificationTools.cpp:46-128 -> (picked indices in pick order, the strengths with every class not picked at 0)"""
    s = [float(v) for v in strengths]
    strong = []
    for _ in range(len(s)):                       # :58-80
        best, best_at = 0.0, -1
        for j, w in enumerate(s):
            if w > min_default and w >= best and j not in strong:
                best, best_at = w, j
        if best_at == -1:
            break
        strong.append(best_at)
    if not strong and s:                          # :83-90: std::max_element returns the first maximum
        at = 0
        for j in range(1, len(s)):
            if s[at] < s[j]:
                at = j
        if s[at] > min_fallback:
            strong.append(at)
    if strong and strong[0] == none:              # :101-106
        strong = []
    strong = [c for c in strong if c != none]     # :108-116
    return strong, [v if i in strong else 0.0 for i, v in enumerate(s)]   # :119-125


def correlation(x1, x2):
    """TStatistics::Correlation, Statistics.cpp:604-638"""
    length = len(x1)
    if not length:
        return 0.0
    ss1 = ss2 = ss11 = ss12 = ss22 = 0.0
    for a, b in zip(x1, x2):
        a, b = float(a), float(b)
        ss12 = ss12 + a * b
        ss1 = ss1 + a
        ss11 = ss11 + a * a
        ss2 = ss2 + b
        ss22 = ss22 + b * b
    ss1 = ss1 / length
    ss2 = ss2 / length
    denom2 = (ss11 - ss1 * ss1 * length) * (ss22 - ss2 * ss2 * length)
    num = ss12 - (ss1 * ss2 * length)
    if abs(denom2) > EPSILON:
        return num / math.sqrt(denom2) if denom2 >= 0.0 else math.nan   # ::sqrt of a negative number: NaN
    return 0.0


def envelope(peaks):
    """the peak frames without leading and trailing silence <= -24 dB (ClassificationHeuristics.cpp:45-76)"""
    n = len(peaks)
    leading = 0
    for f in range(n):                            # :51-58
        if peaks[f] > SILENCE_FLOOR:
            break
        leading += 1
    trailing = 0
    f = n - 1
    while f > leading:                            # :60-67: stops at f > SilentLeadingFrames, as written
        if peaks[f] > SILENCE_FLOOR:
            break
        trailing += 1
        f -= 1
    return [float(peaks[i + leading]) for i in range(n - leading - trailing)]


def fade_out(n):
    """:79-83; n == 1: 0.0 / 0.0, a NaN"""
    out = []
    for i in range(n):
        x = 1.0 - (float(i) / float(n - 1) if n != 1 else math.nan)
        out.append(math.pow(x, 4.0) if x == x else math.nan)
    return out


def is_oneshot(length, onsets, peaks):
    """ClassificationHeuristics.cpp:12-98 -> (result, confidence)"""
    if length < 0.5:
        return True, 0.85
    if length < 1 and onsets <= 2:
        return True, 0.75
    length_confidence = math.pow(1.0 - (std_min(4.0, std_max(0.0, length - 1.0)) / 4.0), 0.5)
    env = envelope(peaks)
    c = correlation(fade_out(len(env)), env)
    envelope_confidence = std_min(1.0, abs(c))
    confidence = length_confidence * 0.3 + envelope_confidence * 0.7
    return confidence > 0.7, confidence


def is_loop(length, onsets, percussive_confidence, complex_confidence, flux_mean):
    """ClassificationHeuristics.cpp:102-149 -> (result, confidence)"""
    if onsets < 8:
        return False, 0.0
    if flux_mean > 0.9:
        return False, 0.0
    length_confidence = math.pow(std_max(0.0, std_min(4.0, length - 1.0) / 4.0), 0.5)
    rhythm_confidence = 0.0
    if percussive_confidence > 0.25 and complex_confidence > 0.25:
        rhythm_confidence = std_min(1.0, percussive_confidence * 2.0)
    confidence = length_confidence * 0.3 + rhythm_confidence * 0.7
    return confidence > 0.7, confidence


def decide(peaks, scalars, class_signature=None, category_signature=None, loop_class=0, oneshot_class=1, use_heuristics=True,
           none_category=-1, dead=False):
    """one file (SA:1081-1231).  scalars: the five of SCALARS.  -> dict with the members of afx_decision_out (picks -1 padded)
    and "margins": the values a rounding could turn the decision on -- see margin()"""
    length, onsets, percussive, complex_, flux = (float(v) for v in scalars)
    k = 0 if category_signature is None else len(category_signature)
    out = {"confidences": [-1.0, -1.0], "flags": 0, "class_strengths": [0.0, 0.0], "classes": [-1, -1],
           "category_strengths": [0.0] * k, "categories": [-1] * k, "model_strengths": None, "pick_strengths": [],
           "category_pick_strengths": []}
    if dead or len(peaks) == 0:
        return out
    classes = []
    if class_signature is not None:
        s = category_strengths(class_signature)
        out["model_strengths"] = list(s)
        if use_heuristics:
            one, out["confidences"][0] = is_oneshot(length, onsets, peaks)
            if one:
                out["flags"] |= IS_ONESHOT
                if s[loop_class] > s[oneshot_class]:          # SA:1123-1133
                    out["flags"] |= OVERRIDDEN
                    s[loop_class] = m_min(out["confidences"][0] / 2, s[loop_class])
                    s[oneshot_class] = out["confidences"][0]
            else:
                loop, out["confidences"][1] = is_loop(length, onsets, percussive, complex_, flux)
                if loop:
                    out["flags"] |= IS_LOOP
                    if s[loop_class] < s[oneshot_class]:      # SA:1137-1147
                        out["flags"] |= OVERRIDDEN
                        s[loop_class] = out["confidences"][1]
                        s[oneshot_class] = m_min(out["confidences"][1] / 2, s[oneshot_class])
        out["pick_strengths"] = list(s)
        classes, out["class_strengths"] = pick_all_strong(s)
        out["classes"] = classes + [-1] * (2 - len(classes))
    if category_signature is not None and (not classes or oneshot_class in classes):   # SA:1202-1224
        s = category_strengths(category_signature)
        out["category_pick_strengths"] = list(s)
        picked, out["category_strengths"] = pick_all_strong(s, none_category)
        out["categories"] = picked + [-1] * (k - len(picked))
    return out


def margin(result):
    """how far the decision of `result` (decide's) lies from every comparison a rounding of the device's confidences and
    strengths could turn: the evaluated confidences from 0.7, the two class strengths from one another (the override's test
    and the pick's order), every strength that goes to a pick from 0.2 and from 0.01"""
    gaps = [abs(c - 0.7) for c in result["confidences"] if c not in (-1.0, 0.0, 0.85, 0.75)]
    if result["model_strengths"] is not None:
        gaps.append(abs(result["model_strengths"][0] - result["model_strengths"][1]))
        gaps.append(abs(result["pick_strengths"][0] - result["pick_strengths"][1]))
    for v in result["pick_strengths"] + result["category_pick_strengths"]:
        gaps += [abs(v - MIN_DEFAULT_WEIGHT), abs(v - MIN_FALLBACK_WEIGHT)]
    return min(gaps) if gaps else math.inf
