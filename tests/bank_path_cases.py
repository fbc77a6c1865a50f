"""Channel banks that take every branch of tree_kernel.hpp the bank planner can plan, on both engines.

Which branches of tree_kernel run is decided by the tables the planner (sdrangel_amd/csrc/chan_plan.cpp) writes, not by the code:
tests/chan_plan_paths.cpp plans a bank on the host and names the branches its tables select (the names are explained there).
VOCAB is every name; UNREACHABLE says, per engine, which of them no plan can select and why.  CASES are the banks
tests/test_bank_paths_gpu.py runs on the GPU; each one lists, per engine, the paths it is there for, and
tests/test_bank_paths.py checks that it still takes them and that together the cases take every reachable path.

The cases are what `python -m tests.bank_path_cases` prints: two fixed banks (the deepest chain a test-sized feed still gets a few
dozen outputs from at 61.44 MS/s, and a single pass of seven levels over the raw stream), then a greedy cover of the paths by
seeded random banks (random_bank(), seed SEARCH_SEED)."""
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdrangel_amd", "csrc")

# planner options: None = the defaults, else (SDRX_CHAN_MAX_LEVELS, SDRX_CHAN_LDS_KB) -- the two deep-pass sets of test_chan_gpu.py
OPTIONS = {"default": None, "deep8": (8, 80), "deep10": (10, 150)}
ENGINES = ("mfma", "valu")

ARMS = ("none", "EO", "EA", "EOA")
SINKS = ("none", "end", "stream", "list")
VOCAB = sorted(
    [f"mfma.fast.k{k}" for k in range(4)]
    + [f"mfma.{c}.{a}.{s}" for c in ("centre", "lower", "upper") for a in ARMS for s in SINKS]
    + ["mfma.lower.absent", "mfma.upper.absent", "mfma.tail"]
    + ["dot2.R8", "dot2.R4", "dot2.R2"]
    + [f"dot2.{h}.{a}.{s}" for h in ("a", "b") for a in ARMS for s in SINKS] + ["dot2.b.absent"]
    + ["root.EO", "root.EA", "root.EOA", "root.bias", "root.nobias"]
    + ["warm.1", "warm.2", "warm.3+", "passes.1", "passes.2-5", "passes.6+"])


def _unreachable(engine):
    out = {}
    for p in VOCAB:
        f = p.split(".")
        if engine == "valu" and f[0] == "mfma":
            out[p] = "the valu engine runs every level on dot2"
        elif len(f) == 4 and f[2] == "none" and f[3] == "none":
            out[p] = "a planned stage writes arms or has a sink (a child that is not there is 'absent')"
        elif len(f) == 4 and f[2] != "none" and f[3] == "stream":
            out[p] = "node streams leave only from a pass's last level, whose stages write no arms"
        elif f[:2] == ["mfma", "centre"] and f[2] in ("EA", "EOA"):
            out[p] = "a centre stage keeps the band's middle, which its channels straddle: its children are centre stages only"
        elif p == "root.bias" and engine == "valu":
            out[p] = "root_xm is set only when level 1 runs on the matrix cores"
        elif p == "root.nobias" and engine == "mfma":
            out[p] = "on the mfma engine level 1 always runs on the matrix cores (2048 outputs per entry and chunk)"
    return out


UNREACHABLE = {e: _unreachable(e) for e in ENGINES}
REACHABLE = {e: sorted(set(VOCAB) - set(UNREACHABLE[e])) for e in ENGINES}

IN_RATES = (2_400_000, 10_000_000, 61_440_000)
_RATES_ABS = (600_000, 300_000, 200_000, 48_000, 25_000, 12_500, 8_000, 2_000, 300)


def random_bank(rng):
    """(in_rate, [(rate, centre)]): 1-40 channels of mixed widths, now and then a second channel on an earlier one's settings"""
    ir = int(rng.choice(IN_RATES))
    rates = [ir // 2, ir // 4] + [r for r in _RATES_ABS if r < ir // 4]
    ch = []
    for _ in range(int(rng.integers(1, 41))):
        if ch and rng.random() < 0.1:
            ch.append(ch[int(rng.integers(0, len(ch)))])
            continue
        r = int(rng.choice(rates))
        ch.append((r, int(rng.integers(-ir // 2 + r // 2, ir // 2 - r // 2 + 1))))
    return ir, ch


def build_lister(out_dir):
    exe = os.path.join(out_dir, "chan_plan_paths")
    # plain g++ as tests/test_chan_planner.py builds chan_plan_check.cpp: host-only planner, flags as in csrc/Makefile
    subprocess.check_call(["g++", "-O3", "-std=c++17", "-ffp-contract=off", "-Wall", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "chan_plan_paths.cpp"), os.path.join(CSRC, "chan_plan.cpp"), "-o", exe])
    return exe


def lister_line(engine, options, in_rate, channels):
    ml, kb = OPTIONS[options] or (0, 0)
    return f"{engine} {kb} {ml} {in_rate} {len(channels)} " + " ".join(f"{i} {r} {f}" for i, (r, f) in enumerate(channels))


def run_lister(exe, lines):
    """one {"error", "paths"} per line"""
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300, check=True)
    res = [json.loads(s) for s in out.stdout.splitlines()]
    assert len(res) == len(lines)
    return res


def case_paths(exe, case):
    """{engine: set of paths} of one case"""
    lines = [lister_line(e, case["options"], case["in_rate"], case["channels"]) for e in ENGINES]
    res = run_lister(exe, lines)
    for r in res:
        assert r["error"] == "", (case["name"], r["error"])
    return {e: set(r["paths"]) for e, r in zip(ENGINES, res)}


CASES = [
    dict(name="deep17_61M", in_rate=61440000, options="default",
         channels=[(25000, 10317472), (600000, -10200633), (2000, 13238937), (600000, -11596075), (15360000, -19907103),
                   (300000, -5029611), (15360000, 15501352), (15360000, 15501352), (600000, 28836842), (600000, 29051838),
                   (600000, -12453365), (8000, -2802347), (25000, 19912467), (2000, 15294644), (300, -25474922),
                   (15360000, 15501352), (200000, -5262624), (8000, -604668), (8000, -25136833), (12500, 8266792),
                   (2000, 13238937), (8000, -3871608), (8000, 13175398), (8000, 1820685), (25000, -15526705),
                   (300, -11207008), (30720000, 12351164), (600000, -23198657), (8000, -5652040), (8000, -4964182),
                   (8000, 13175398), (2000, -8991802), (300, 10435949), (2000, 24759714), (200000, -1135541),
                   (300, 15298134), (8000, -2802347), (8000, -7799892)],
         paths={"mfma": ["mfma.centre.EO.end", "mfma.centre.EO.none", "mfma.centre.none.end", "mfma.centre.none.list",
                          "mfma.centre.none.stream", "mfma.fast.k1", "mfma.fast.k3", "mfma.lower.EA.end",
                          "mfma.lower.EA.none", "mfma.lower.EO.none", "mfma.lower.EOA.none", "mfma.lower.absent",
                          "mfma.lower.none.end", "mfma.lower.none.list", "mfma.lower.none.stream", "mfma.tail",
                          "mfma.upper.EA.list", "mfma.upper.EA.none", "mfma.upper.EO.none", "mfma.upper.absent",
                          "mfma.upper.none.end", "mfma.upper.none.list", "mfma.upper.none.stream", "passes.6+", "root.EA",
                          "root.EO", "root.EOA", "root.bias", "warm.1"],
                "valu": ["dot2.R2", "dot2.R4", "dot2.R8", "dot2.a.EA.end", "dot2.a.EA.none", "dot2.a.EO.end",
                          "dot2.a.EO.none", "dot2.a.EOA.none", "dot2.a.none.end", "dot2.a.none.list", "dot2.a.none.stream",
                          "dot2.b.EA.list", "dot2.b.EA.none", "dot2.b.EO.none", "dot2.b.absent", "dot2.b.none.end",
                          "dot2.b.none.list", "dot2.b.none.stream", "passes.6+", "root.EA", "root.EO", "root.EOA",
                          "root.nobias", "warm.1"]}),
    dict(name="warm2_raw", in_rate=2400000, options="deep8",
         channels=[(600000, -449273), (1200000, 34809), (1200000, 34809), (200000, -115156), (200000, -1001864),
                   (1200000, 128193), (8000, -38599), (8000, -38599), (300000, 267301), (200000, -8688), (300000, -262915),
                   (600000, 566908), (8000, 786256), (1200000, -550890), (300000, 650058), (8000, 786256),
                   (600000, -467224), (48000, -691290), (1200000, 158995), (8000, -662464), (600000, -467224),
                   (25000, -662244), (48000, -208113), (48000, 1127442), (200000, 262734), (600000, -467224),
                   (200000, 678640), (12500, -328098)],
         paths={"mfma": ["dot2.R2", "dot2.a.EA.end", "dot2.a.EA.none", "dot2.a.EO.none", "dot2.a.none.end",
                          "dot2.a.none.list", "dot2.b.absent", "mfma.lower.EA.list", "mfma.lower.EO.end",
                          "mfma.upper.EA.end", "mfma.upper.EOA.end", "passes.1", "warm.2"],
                "valu": ["dot2.a.EA.list", "dot2.b.EA.end", "dot2.b.EOA.end", "passes.1", "warm.2"]}),
    dict(name="cover1", in_rate=2400000, options="deep10",
         channels=[(200000, -891685), (600000, -361585), (600000, 366665), (8000, -147463), (600000, 366665),
                   (300, -680288), (300000, -13592), (2000, 370218), (1200000, -589767), (25000, 479076),
                   (200000, -1039032), (200000, 935932), (12500, 414348), (200000, -1058757), (1200000, 523385),
                   (8000, -3154), (25000, 4347), (8000, 891576), (300000, -13592), (200000, -69021), (8000, 139235),
                   (300, -811554), (200000, 594097), (12500, -717449), (8000, -380725), (200000, -636689), (48000, -377890),
                   (12500, -237780), (25000, -865173), (600000, -15625), (48000, 571908), (1200000, 74238),
                   (300000, -871097), (48000, 63808), (2000, 676082)],
         paths={"mfma": ["dot2.R4", "dot2.a.EO.end", "dot2.a.EOA.none", "dot2.a.none.stream", "dot2.b.EA.none",
                          "dot2.b.EO.none", "dot2.b.none.end", "mfma.centre.EO.list", "mfma.lower.EOA.end",
                          "mfma.upper.EOA.list", "mfma.upper.EOA.none", "passes.2-5", "warm.3+"],
                "valu": ["dot2.a.EO.list", "dot2.a.EOA.end", "dot2.b.EOA.list", "dot2.b.EOA.none", "passes.2-5", "warm.3+"]}),
    dict(name="cover2", in_rate=2400000, options="deep8",
         channels=[(12500, -962387), (300, 296186), (1200000, 135805), (48000, -345874), (48000, -345874), (12500, -962387),
                   (2000, -853776), (300000, -990493), (8000, 782513), (12500, 547384), (25000, 967584), (25000, -918353),
                   (8000, -919624), (300, -491122), (2000, -1132958), (600000, 729910), (600000, 729910), (1200000, 2515),
                   (25000, -1169142), (2000, 1198324), (200000, 213831), (200000, 13052), (200000, 783581),
                   (600000, -800155), (200000, -263305), (25000, 268201), (200000, 792515), (48000, 712337),
                   (12500, 513393), (300000, 328785), (600000, -232023), (8000, 782513), (48000, 747492), (200000, 210283),
                   (48000, 488180), (300, 183574)],
         paths={"mfma": ["dot2.b.EO.end", "dot2.b.EOA.none", "mfma.fast.k2", "mfma.lower.EOA.list"],
                "valu": ["dot2.a.EOA.list", "dot2.b.EO.end"]}),
    dict(name="cover3", in_rate=2400000, options="deep8",
         channels=[(12500, -739599), (12500, -739599), (48000, -98462), (12500, -739599), (12500, 1052961), (2000, -453016),
                   (600000, 232643), (300000, -247504), (200000, -1058789), (1200000, -402709), (8000, -1169125),
                   (2000, 475029), (8000, 1050986), (48000, -175752), (300, 523638), (300, 851130), (12500, -76024),
                   (48000, 696706), (600000, 538581), (1200000, 52007), (48000, -98462), (48000, -397865), (48000, -566425),
                   (12500, 172309), (2000, 83039), (12500, -295142), (200000, -951335), (12500, 511349), (12500, 1151850),
                   (200000, 8849), (8000, -740263), (2000, 313343), (12500, -877262), (300000, -777284), (48000, -127914),
                   (48000, -1103944)],
         paths={"mfma": ["dot2.a.EO.list", "dot2.b.EA.end", "mfma.upper.EO.list"],
                "valu": ["dot2.b.EO.list"]}),
    dict(name="cover4", in_rate=2400000, options="deep8",
         channels=[(8000, 315105), (12500, 131011), (300, 166954), (1200000, -236179), (200000, -1090389), (2000, 499418),
                   (48000, 846644), (2000, 1184658), (12500, -1070242), (300000, 866574), (1200000, -259816),
                   (25000, 453751), (48000, -1059837), (300, -549109), (300000, 314992), (48000, -61792), (48000, -556430),
                   (12500, -1070242), (25000, 185131), (1200000, -236179), (300000, -344312), (8000, 822569),
                   (25000, 1128834), (8000, -1161352), (2000, -898550), (8000, -958682), (12500, -1070242),
                   (48000, 1066017), (300000, 213378), (300, -633797), (8000, 1191900), (300, 312126), (2000, -131212),
                   (8000, -477488), (25000, -555422), (48000, 1007293)],
         paths={"mfma": ["dot2.R8", "dot2.a.EA.list", "mfma.upper.EO.end"],
                "valu": []}),
    dict(name="cover5", in_rate=2400000, options="deep8",
         channels=[(25000, -1127140), (1200000, 335090), (2000, 672389), (1200000, 335090), (200000, -433166),
                   (8000, -832351), (2000, -416986), (12500, 646616), (1200000, -462484), (600000, -556651),
                   (300000, 311001), (48000, 874254), (1200000, 101335), (25000, 808980), (600000, -234997),
                   (48000, -450159), (2000, 150735), (200000, 271530), (1200000, 335090), (2000, 1138113), (300000, 11858),
                   (300000, -502140), (12500, -300427), (48000, -68572), (600000, -326118), (48000, -68572),
                   (300000, -650697), (48000, 1257), (25000, -222969), (2000, -723472), (2000, 965149), (2000, 965149),
                   (48000, -1021722), (2000, -873549), (600000, -54824)],
         paths={"mfma": ["dot2.b.none.stream", "mfma.fast.k0"],
                "valu": []}),
    dict(name="cover6", in_rate=2400000, options="deep8",
         channels=[(2000, 561602), (1200000, -415739), (12500, 67108), (12500, 841577), (1200000, -258250), (300000, 72624),
                   (2000, 561602), (1200000, -200952), (8000, -949793), (48000, -329115), (8000, -1125077), (2000, 1071221),
                   (300000, -515567), (300000, -126589), (48000, -329115), (12500, -188202), (300000, 72624),
                   (300000, -556074), (25000, -691572), (200000, 795369), (600000, 694958), (12500, -459758),
                   (12500, 841577), (2000, -434585), (200000, 199643), (8000, 741704), (300000, 61129), (25000, 574709),
                   (2000, 597669)],
         paths={"mfma": ["dot2.a.EOA.end", "dot2.b.none.list"],
                "valu": []}),
    dict(name="cover7", in_rate=2400000, options="deep8",
         channels=[(600000, -703501), (48000, -976444), (600000, 558844), (48000, -976444), (8000, -443810),
                   (12500, -371011), (200000, 757007), (48000, 771488), (200000, 757007), (300000, -601354), (48000, 771488)],
         paths={"mfma": ["mfma.lower.EO.list"],
                "valu": []}),
    dict(name="cover8", in_rate=2400000, options="deep8",
         channels=[(300000, 932641), (2000, -566769), (1200000, 185754), (25000, 395870), (300000, -522830),
                   (200000, 866179), (48000, 944775), (48000, -482703), (2000, 709544), (25000, 835812), (48000, -482703),
                   (25000, 424701), (12500, -568119), (12500, -491370), (48000, -482703), (12500, 858257), (2000, -616920),
                   (200000, 377192), (25000, -396994), (8000, 379207)],
         paths={"mfma": ["dot2.b.EO.list"],
                "valu": []}),
    dict(name="cover9", in_rate=2400000, options="deep8",
         channels=[(600000, 639089), (8000, 911184), (300000, -693702), (25000, -357890), (1200000, -212958),
                   (48000, -796764), (8000, -829252), (1200000, 48858), (200000, -536790), (2000, -808383), (200000, 37709),
                   (600000, 343971), (200000, -265324), (48000, -790373), (200000, 325862), (48000, -790373),
                   (600000, 639089), (300000, -550719), (8000, -829252), (600000, 692765), (25000, 24113), (2000, 127490),
                   (2000, -808383), (200000, -757834), (25000, -114295)],
         paths={"mfma": ["dot2.b.EA.list"],
                "valu": []}),
    dict(name="cover10", in_rate=2400000, options="deep8",
         channels=[(1200000, -186614), (12500, -663442), (12500, -503790), (25000, -489441), (8000, -554993),
                   (600000, -801575), (600000, -801575), (12500, -784184), (48000, -793023), (8000, -304006),
                   (300000, -688400), (2000, -493474), (600000, 694325), (8000, -34849), (300000, -544673),
                   (25000, -748669), (600000, 802856), (25000, 731764), (48000, -749753), (2000, 662835), (8000, -766652),
                   (8000, 1038692), (25000, -843067), (300000, -203988), (12500, 1099605), (12500, 625840), (2000, 662835),
                   (600000, -67409), (2000, 662835), (600000, -647351), (300000, 671129), (600000, -610703),
                   (600000, -801575), (48000, -105424), (12500, 721418), (600000, -858201), (300000, 586450)],
         paths={"mfma": ["dot2.b.EOA.end"],
                "valu": []}),
    dict(name="cover11", in_rate=2400000, options="deep8",
         channels=[(300000, -428480), (300000, 94191), (8000, -901190), (48000, -791707), (300, 203020), (48000, -791707),
                   (12500, -848779), (200000, 594084), (8000, -804062), (600000, -886537), (200000, -1086154),
                   (300000, 580160), (12500, 931072), (300000, -771400), (8000, -787944), (48000, 848790), (200000, 158800),
                   (600000, -676203), (48000, 1159637), (300, 781217), (8000, 1161971), (25000, 511329)],
         paths={"mfma": ["dot2.b.EOA.list"],
                "valu": []}),
    dict(name="cover12", in_rate=2400000, options="deep8",
         channels=[(25000, -251044), (25000, -5957), (25000, -251044), (2000, 144819), (200000, 744769), (2000, 841429),
                   (48000, -448233), (48000, -374666), (2000, 752067), (25000, 1124235), (25000, 1119090), (300000, 147079),
                   (600000, 663433), (300, -288142), (48000, 78043), (25000, -251044), (300, 159762), (300000, -946147),
                   (2000, -1042585), (8000, 504756), (8000, -432642), (48000, -448233), (12500, -1008413), (200000, 160121),
                   (25000, -261419), (12500, -22243)],
         paths={"mfma": ["dot2.a.EOA.list"],
                "valu": []}),
]

SEARCH_SEED = 2026


def search(exe, n_banks=20000):
    """The case list: two fixed picks, then a greedy cover of every reachable path of both engines by seeded random banks
    under every option set (most new paths first; ties: the shallower, then the smaller bank).  Each case claims what it added."""
    rng = np.random.default_rng(SEARCH_SEED)
    banks = [random_bank(rng) for _ in range(n_banks)]
    cands = [(o, ir, ch) for ir, ch in banks for o in OPTIONS]
    res = run_lister(exe, [lister_line(e, o, ir, ch) for o, ir, ch in cands for e in ENGINES])
    pool = []
    for i, (o, ir, ch) in enumerate(cands):
        r = res[2 * i: 2 * i + 2]
        if r[0]["error"] or r[1]["error"]:
            continue
        pool.append(dict(options=o, in_rate=ir, channels=ch, depth=r[0]["depth"],
                         pairs={(e, p) for e, x in zip(ENGINES, r) for p in x["paths"]}))
    want = {(e, p) for e in ENGINES for p in REACHABLE[e]}
    cases, have = [], set()

    def pick(name, ok):
        best = max((c for c in pool if ok(c)), key=lambda c: (len(c["pairs"] & want - have), -c["depth"], -len(c["channels"])))
        new = best["pairs"] & want - have
        have.update(new)
        cases.append(dict(name=name, in_rate=best["in_rate"], channels=best["channels"], options=best["options"],
                          paths={e: sorted(p for f, p in new if f == e) for e in ENGINES}))

    # the deepest chain a test-sized feed (5 M samples) still gets a few dozen outputs from at 61.44 MS/s: 17 stages, 40 outputs;
    # with more than five passes per feed
    pick("deep17_61M", lambda c: c["in_rate"] == 61_440_000 and c["depth"] == 17 and c["options"] == "default"
         and ("mfma", "passes.6+") in c["pairs"])
    # one pass of seven levels (warm = 2) over the raw stream, so that its warm-up chunks are input samples
    pick("warm2_raw", lambda c: c["depth"] == 7 and ("mfma", "warm.2") in c["pairs"] and ("mfma", "passes.1") in c["pairs"])
    while want - have:
        pick(f"cover{len(cases) - 1}", lambda c: c["depth"] <= 12)           # feeds of ~1 M samples give every channel outputs
    return cases


if __name__ == "__main__":
    import tempfile
    print(json.dumps(search(build_lister(tempfile.mkdtemp())), indent=1))
