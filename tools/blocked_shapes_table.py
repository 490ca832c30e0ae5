"""One line per case from the per-solution log of tests/test_blocked_shapes_{cpu,gpu}.py (HIPMF_FRONT_SHAPES_LOG=<file> while they run):
the shape asked for and reached, and per call family the worst omega / max(omega_lapack, eps) and fe / max(fe_lapack, eps cond_inf) over
the case's solutions (entries of the inverse: the forward error alone), then the worst ratio of every family over all cases.
    python tools/blocked_shapes_table.py <log>  >  table      (the table parts of profiles/r23_blocked_shapes.txt)"""
import re
import sys

EPS = 2.220446049250313e-16
FAMILIES = [("transpose_many (host)", "tm-host"), ("transpose_many (device)", "tm-dev"), ("transpose_many conjugate 0", "z-tm-T"), ("transpose_many conjugate 1", "z-tm-H"),
            ("sparse transposed", "sp-T"), ("sparse trans 0", "z-sp-A"), ("sparse trans 1", "z-sp-T"), ("sparse trans 2", "z-sp-H"), ("sparse", "sp-A"),
            ("inverse_entries by rows", "inv-rows"), ("inverse_entries", "inv-cols"), ("many col", "z-many")]
cases, order, worst = {}, [], {}
for l in open(sys.argv[1]):
    l = l.rstrip("\n")
    m = re.match(r"^(.*?)\s+n (\d+) asked (.*) reached (.*)$", l)
    if m:
        name = m.group(1).strip()
        if name not in cases:
            order.append(name)
        cases[name] = {"n": m.group(2), "asked": m.group(3), "reached": m.group(4), "fam": {}, "k": 0, "cond": 0.0}
        continue
    m = re.search(r"(?:omega (\S+) omega_lapack (\S+) |entries \d+ )fe (\S+) fe_lapack (\S+) cond_inf (\S+)", l)
    if not m:
        continue
    for key, fam in FAMILIES:
        at = l.find(" " + key)
        if at >= 0:
            break
    else:
        continue
    name = re.sub(r" \[(big leaf|leaf under the root)\]$", "", l[:at].strip())
    c = cases[name]
    fe, fel, cond = float(m.group(3)), float(m.group(4)), float(m.group(5))
    ro = float(m.group(1)) / max(float(m.group(2)), EPS) if m.group(1) else 0.0
    rf = fe / max(fel, EPS * cond)
    c["k"] += 1
    c["cond"] = max(c["cond"], cond)
    o, f = c["fam"].get(fam, (0.0, 0.0))
    c["fam"][fam] = (max(o, ro), max(f, rf))
    for kind, r in (("omega", ro), ("fe", rf)):
        if r > worst.get((fam, kind), (0.0, ""))[0]:
            worst[(fam, kind)] = (r, name)


def short(d):
    return re.sub(r"[{}',]", "", d).replace("nsuper: ", "ns ").replace("max_front: ", "f ").replace("max_pivots: ", "p ").replace("mid_fronts: ", "mid ")\
        .replace("wave_fronts: ", "wave ").replace("leaf_fronts: ", "leaf ").replace("symmetric_ldlt: ", "ldlt ")


order = [n for n in order if cases[n]["k"] > 0]  # (a case that failed before its first solution has no figures)
print("# %d cases, %d solutions checked, largest cond_inf = %.0f" % (len(order), sum(cases[n]["k"] for n in order), max(cases[n]["cond"] for n in order)))
print("# worst ratio per call family: omega / max(omega_lapack, eps) (case), fe / max(fe_lapack, eps cond_inf) (case)")
for _, fam in FAMILIES:
    if (fam, "fe") in worst:
        o, f = worst.get((fam, "omega"), (0.0, "-")), worst[(fam, "fe")]
        print(("#   %-9s fe %.2f (%s)" % (fam, f[0], f[1])) if fam.startswith("inv") else "#   %-9s omega %.2f (%s), fe %.2f (%s)" % (fam, o[0], o[1], f[0], f[1]))
print("# case | n | asked | reached | solutions | family omega-ratio/fe-ratio ... | cond_inf")
for n in order:
    c = cases[n]
    fams = " ".join(("%s -/%.2f" % (fam, c["fam"][fam][1])) if fam.startswith("inv") else "%s %.2f/%.2f" % (fam, c["fam"][fam][0], c["fam"][fam][1]) for _, fam in FAMILIES if fam in c["fam"])
    print("%s | %s | %s | %s | %d | %s | %.0f" % (n, c["n"], short(c["asked"]), short(c["reached"]), c["k"], fams, c["cond"]))
