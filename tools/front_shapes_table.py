"""One line per case from the per-solution log of tests/test_front_shapes_gpu.py (HIPMF_FRONT_SHAPES_LOG=<file> while it runs):
the shape asked for and reached, and the worst omega / omega_lapack and forward error / LAPACK's over the case's solutions.
    python tools/front_shapes_table.py <log>  >  table      (the table part of profiles/r08_front_shapes.txt)"""
import re
import sys

EPS = 2.220446049250313e-16
cases, order = {}, []
for l in open(sys.argv[1]):
    l = l.rstrip("\n")
    m = re.match(r"^(.*?)\s+n (\d+) asked (.*) reached (.*)$", l)
    if m:
        name = m.group(1).strip()
        cases[name] = {"n": m.group(2), "asked": m.group(3), "reached": m.group(4), "wo": None, "wf": None, "k": 0}
        order.append(name)
        continue
    m = re.match(r"^(.*?) (\[(?:default|level-set)\] .*?|solve|transpose)\s+omega (\S+) omega_lapack (\S+) fe (\S+) fe_lapack (\S+) cond_inf (\S+)", l)
    if not m:
        continue
    name, what = m.group(1).strip(), m.group(2)
    om, oml, fe, fel, cond = map(float, m.groups()[2:])
    c = cases[name]
    c["k"] += 1
    c["cond"] = cond
    ro, rf = om / max(oml, EPS), fe / max(fel, EPS * cond)
    c["maxoml"] = max(c.get("maxoml", 0.0), oml)
    if c["wo"] is None or ro > c["wo"][0]:
        c["wo"] = (ro, what, om, oml)
    if c["wf"] is None or rf > c["wf"][0]:
        c["wf"] = (rf, what, fe, fel)
def short(d):
    return re.sub(r"[{}',]", "", d).replace("nsuper: ", "ns ").replace("max_front: ", "f ").replace("max_pivots: ", "p ").replace("mid_fronts: ", "mid ").replace("wave_fronts: ", "wave ").replace("leaf_fronts: ", "leaf ")\
        .replace("symmetric_ldlt: ", "ldlt ")
order = [n for n in dict.fromkeys(order) if cases[n]["k"] > 0]  # (a case that failed before its first solution has no figures)
cases = {n: cases[n] for n in order}
wo = max((c["wo"][0], n) for n, c in cases.items())
wf = max((c["wf"][0], n) for n, c in cases.items())
print("# %d cases, %d solutions checked; largest omega / max(omega_lapack, eps) = %.2f (%s), largest fe / max(fe_lapack, eps cond) = %.2f (%s)" % (len(order), sum(c["k"] for c in cases.values()), wo[0], wo[1], wf[0], wf[1]))
print("# largest omega_lapack = %.2f eps, largest cond_inf = %.0f" % (max(c["maxoml"] for c in cases.values()) / EPS, max(c["cond"] for c in cases.values())))
print("# case | n | asked | reached | solutions | worst omega: ratio, which solve, omega, omega_lapack | worst fe: ratio, which solve, fe, fe_lapack | cond_inf")
for n in order:
    c = cases[n]
    print("%s | %s | %s | %s | %d | %.2f %s %.3e %.3e | %.2f %s %.3e %.3e | %.0f" % (n, c["n"], short(c["asked"]), short(c["reached"]), c["k"], c["wo"][0], c["wo"][1], c["wo"][2], c["wo"][3], c["wf"][0], c["wf"][1], c["wf"][2], c["wf"][3], c["cond"]))
