"""Generate the committed fixtures of the incucyte_population parity tests.

Run where the reference sources lie (REF, default /root/reference):
    python tests/golden/make_incucyte_fixtures.py

It compiles the vendored CVODE 5.3.0 and Eigen from the reference tree, where they lie, together with
tests/golden/incucyte_ref_driver.cpp and oracle/eigen_ls.cpp into oracle/_ref/incucyte/ -- twice, as
oracle/Makefile builds its two reference libraries: with FMA contraction (the reference's own build
flags) and with -ffp-contract=off (the arithmetic the device follows). Nothing of the reference is
copied into the repository; only this script's and the driver's own text and the data are committed:

  incucyte_data.json / incucyte_data.nc   synthetic drug-response data (JSON sidecar and classic netCDF
                                          of the reference's drug_response_data.nc schema): E = 2
                                          experiments, 9 concentrations, 4 replicates, simulated at TRUE
                                          with seeded Student-t(3) noise, one NaN observation
  incucyte_data_e1.json                   experiment 1 alone
  incucyte_prior.xml, incucyte_prior_e1.xml, incucyte_likelihood*.xml
  incucyte_golden.npz                     64 prior draws (seed 20261019) + hand-made rows reaching every
                                          branch, with logp of both builds, the no-FMA build's simulated
                                          wells, CTB, per-well step counts and return codes, and the
                                          spread between the two builds (the parity tests' tolerance)
`--check` regenerates the rows with the built drivers and compares them with the committed file.
`--time` prints the single-threaded time per evaluation of the driver.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import struct
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("REF", "/root/reference")
OUT = os.path.join(ROOT, "oracle", "_ref", "incucyte")
DRUG, CELL_LINE = "drugA", "lineX"

# (name, value the data are simulated at, prior lower, prior upper); the first 31 in the order of
# BCM3HIP_INC_* (include/bcm3hip.h)
VARIABLES = [
    ("sigma_confluence", 2.0, 1.0, 4.0), ("sigma_apoptosis_marker", 0.5, 0.2, 1.0), ("sigma_ctb", 0.1, 0.05, 0.3),
    ("pao_apoptosis_rate", 0.2, 0.05, 0.5),
    ("drug_proliferation_rate_ic50", -0.5, -1.5, 0.5), ("drug_proliferation_rate_steepness", 1.0, 0.0, 2.0),
    ("drug_proliferation_rate_maxeffect", 0.8, 0.3, 1.0),
    ("drug_apoptosis_rate_ic50", 0.0, -1.0, 1.0), ("drug_apoptosis_rate_steepness", 1.0, 0.0, 2.0),
    ("drug_apoptosis_rate_maxeffect", 0.05, 0.0, 0.1),
    ("proliferation_rate", 0.035, 0.02, 0.05), ("apoptosis_rate", 0.05, 0.01, 0.1), ("apoptosis_duration", 8.0, 2.0, 20.0),
    ("apoptosis_remove_rate", 0.1, 0.02, 0.3),
    ("log10_cell_size", 2.8, 2.6, 3.0), ("pao_apoptotic_cell_size", 0.5, 0.2, 1.0), ("apoptotic_cell_size", 0.6, 0.2, 1.0),
    ("debris_size", 0.2, 0.05, 0.5), ("apoptosis_marker_size", 0.5, 0.2, 1.0), ("pao_apoptosis_marker_size", 0.6, 0.2, 1.0),
    ("debris_apoptosis_marker_size", 0.3, 0.1, 0.6),
    ("pao_delay", 1.0, 0.0, 4.0), ("pao_effect_time", 4.0, 1.0, 10.0), ("drug_delay", 2.0, 0.0, 6.0),
    ("drug_effect_time", 12.0, 2.0, 24.0),
    ("contact_inhibition_start", 0.5, 0.3, 0.7), ("contact_inhibition_max_confluence", 0.95, 0.8, 1.2),
    ("contact_inhibition_apoptosis_rate", 0.0, 0.0, 1.0),
    ("starting_dead_cell_fraction", 0.05, 0.0, 0.2), ("cell_preadherence_size", 0.5, 0.3, 0.8),
    ("cell_adherence_time", 6.0, 2.0, 12.0),
    ("seeding_density_deviation_1", 0.0, -0.2, 0.2), ("seeding_density_deviation_2", 0.0, -0.2, 0.2),
]
NVARS = 31
NAMES = [v[0] for v in VARIABLES]
TRUE = np.array([v[1] for v in VARIABLES])
LOWER = np.array([v[2] for v in VARIABLES])
UPPER = np.array([v[3] for v in VARIABLES])
NDRAWS, SEED = 64, 20261019

CONCENTRATIONS = [0.01, 0.03, 0.1, 0.3, 1.0, 3.0, 10.0, 30.0, 100.0]
EXPERIMENTS = [  # the first time is 0, one equals the treatment time
    dict(time=[0.0, 6.0, 12.0, 24.0, 30.0, 36.0, 48.0, 60.0, 72.0, 84.0, 96.0, 108.0], treatment_time=24.0,
         ctb_time=108.0, seeding_density=3000.0),
    dict(time=[0.0, 8.0, 16.0, 24.0, 32.0, 40.0, 52.0, 64.0, 76.0, 88.0, 100.0], treatment_time=24.0,
         ctb_time=100.0, seeding_density=4000.0),
]
C_, R_ = 9, 4


def hand_rows():
    """(label, row): rows that reach the branches the prior draws may miss"""
    def row(**kw):
        x = TRUE.copy()
        for k, v in kw.items():
            x[NAMES.index(k)] = v
        return x
    return [
        ("stop_time_before_start", row(pao_delay=-30.0)),                    # CV_ILL_INPUT on the first call: -inf
        ("crosses_contact_inhibition", row(contact_inhibition_start=0.3)),
        ("reaches_max_confluence", row(contact_inhibition_start=0.3, contact_inhibition_max_confluence=0.6,
                                       proliferation_rate=0.05)),
        ("delay_longer_than_experiment", row(apoptosis_duration=500.0)),     # the delay clamps to the first column
        ("history_exhausted", row(apoptosis_remove_rate=40.0, apoptosis_duration=0.05)),  # -inf
        ("negative_control_dies", row(apoptosis_rate=30.0)),                 # CTB = 0 (both builds, both experiments)
        ("zero_effect_time", row(drug_effect_time=0.0)),                     # second stop time at the restart: -inf
        ("truth", TRUE.copy()),
    ]


# ---------------------------------------------------------------------------------------------
def build():
    cv = os.path.join(REF, "dependencies", "cvode-5.3.0")
    eigen = os.path.join(REF, "dependencies", "eigen-3.4-rc1")
    if not os.path.isdir(cv):
        raise SystemExit(f"reference CVODE sources not found at {cv}")
    srcs = ["cvode/cvode.c", "cvode/cvode_io.c", "cvode/cvode_ls.c", "cvode/cvode_nls.c", "cvode/cvode_proj.c",
            "sundials/sundials_math.c", "sundials/sundials_nvector.c", "sundials/sundials_matrix.c",
            "sundials/sundials_linearsolver.c", "sundials/sundials_nonlinearsolver.c",
            "sundials/sundials_nvector_senswrapper.c", "sundials/sundials_dense.c", "sundials/sundials_band.c",
            "sundials/sundials_version.c", "sundials/sundials_futils.c", "nvector/serial/nvector_serial.c",
            "sunmatrix/dense/sunmatrix_dense.c", "sunmatrix/band/sunmatrix_band.c",
            "sunnonlinsol/newton/sunnonlinsol_newton.c"]
    inc = [f"-I{cv}/include", f"-I{cv}/src/sundials", f"-I{cv}/src/cvode"]
    os.makedirs(OUT, exist_ok=True)
    libs = {}
    for tag, extra in (("fma", []), ("nofma", ["-ffp-contract=off"])):
        lib = os.path.join(OUT, f"libincucyteref_{tag}.so")
        libs[tag] = lib
        deps = [os.path.join(HERE, "incucyte_ref_driver.cpp"), os.path.join(ROOT, "oracle", "eigen_ls.cpp"), __file__]
        if os.path.exists(lib) and all(os.path.getmtime(lib) > os.path.getmtime(d) for d in deps):
            continue
        base = ["-O3", "-march=x86-64-v3", "-fPIC", "-w"] + extra
        objs = []
        for s in srcs:
            o = os.path.join(OUT, tag + "_" + s.replace("/", "_") + ".o")
            subprocess.run(["gcc", *base, "-std=gnu11", *inc, "-c", "-o", o, os.path.join(cv, "src", s)], check=True)
            objs.append(o)
        for s, name in ((os.path.join(ROOT, "oracle", "eigen_ls.cpp"), "eigen_ls"),
                        (os.path.join(HERE, "incucyte_ref_driver.cpp"), "driver")):
            o = os.path.join(OUT, f"{tag}_{name}.o")
            subprocess.run(["g++", *base, "-std=c++14", f"-I{eigen}", *inc, "-c", "-o", o, s], check=True)
            objs.append(o)
        subprocess.run(["g++", "-shared", "-o", lib, *objs, "-lm"], check=True)
    return libs


class Driver:
    def __init__(self, path, data, names):
        self.L = C.CDLL(path)
        dp = C.POINTER(C.c_double)
        self.L.incref_create.restype = C.c_void_p
        self.L.incref_create.argtypes = [C.c_int, C.POINTER(C.c_int)]
        self.L.incref_destroy.argtypes = [C.c_void_p]
        self.L.incref_set_experiment.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                                 C.c_double] + [dp] * 9
        self.L.incref_eval.argtypes = [C.c_void_p, dp, C.c_int, dp, dp, dp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        assert self.L.incref_num_variables() == NVARS
        ix = (C.c_int * NVARS)(*[names.index(n) for n in NAMES[:NVARS]])
        groups = experiment_groups(data)
        self.E = len(groups)
        self.Tmax = max(len(g["time"]) for g in groups)
        self.h = self.L.incref_create(self.E, ix)
        self.keep = []
        for e, g in enumerate(groups):
            arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (
                g["time"], np.log10(np.array(g["drug_concentrations"], dtype=np.float64)), nan_array(g["drug_confluence"]),
                nan_array(g["drug_apoptosis_marker"]), nan_array(g["positive_control_confluence"]),
                nan_array(g["positive_control_apoptosis_marker"]), nan_array(g["negative_control_confluence"]),
                nan_array(g["negative_control_apoptosis_marker"]), nan_array(g["cell_titer_blue_norm"]))]
            self.keep.append(arrs)
            T, Cn, R = arrs[2].shape
            self.L.incref_set_experiment(self.h, e, T, Cn, R, names.index(f"seeding_density_deviation_{e + 1}"),
                                         g["treatment_time"], g["seeding_density"],
                                         *[a.ctypes.data_as(dp) for a in arrs])

    def eval(self, x):
        dp = C.POINTER(C.c_double)
        x = np.ascontiguousarray(x, dtype=np.float64)
        logp = C.c_double()
        wells = np.empty((self.E, 5, self.Tmax, 11))
        ctb = np.empty((self.E, 9))
        steps = np.zeros((self.E, 11), dtype=np.int32)
        codes = np.zeros((self.E, 11), dtype=np.int32)
        self.L.incref_eval(self.h, x.ctypes.data_as(dp), self.Tmax, C.byref(logp), wells.ctypes.data_as(dp),
                           ctb.ctypes.data_as(dp), steps.ctypes.data_as(C.POINTER(C.c_int)),
                           codes.ctypes.data_as(C.POINTER(C.c_int)))
        return logp.value, wells, ctb, steps, codes

    def eval_rows(self, X):
        r = [self.eval(x) for x in X]
        return tuple(np.array([q[k] for q in r]) for k in range(5))


def nan_array(a):
    """JSON array (null = NaN) as float64"""
    return np.array(_nan(a), dtype=np.float64)


def _nan(a):
    if isinstance(a, list):
        return [_nan(v) for v in a]
    return np.nan if a is None else a


def experiment_groups(data):
    base = f"{DRUG}.{CELL_LINE}."
    n = len({k[len(base):] for k in data if k.startswith(base)})
    return [data[f"{base}experiment{k + 1}"] for k in range(n)]


# ---------------------------------------------------------------------------------------------
# the netCDF classic format (CDF-2), fixed-size variables only: a group's dimensions, variables and
# numeric attributes are stored under "<group>.<name>" (bcm3_amd/csrc/host/NetCDFClassic.h)
def write_classic(path, data):
    dims, variables, gattrs = [], [], []

    def dim(name, n):
        dims.append((name, n))
        return len(dims) - 1

    for g, members in data.items():
        T, Cn, R = np.array(_nan(members["drug_confluence"])).shape
        d = {"time": dim(f"{g}.time", T), "drug_concentrations": dim(f"{g}.drug_concentrations", Cn),
             "replicates": dim(f"{g}.replicates", R)}
        layout = {"time": ["time"], "drug_concentrations": ["drug_concentrations"],
                  "drug_confluence": ["time", "drug_concentrations", "replicates"],
                  "drug_apoptosis_marker": ["time", "drug_concentrations", "replicates"],
                  "positive_control_confluence": ["time", "replicates"],
                  "positive_control_apoptosis_marker": ["time", "replicates"],
                  "negative_control_confluence": ["time", "replicates"],
                  "negative_control_apoptosis_marker": ["time", "replicates"],
                  "cell_titer_blue_norm": ["drug_concentrations"]}
        for name, v in members.items():
            if name in layout:
                variables.append((f"{g}.{name}", [d[k] for k in layout[name]], np.array(_nan(v), dtype=">f8")))
            else:
                gattrs.append((f"{g}.{name}", float(v)))

    def name(s):
        b = s.encode()
        return struct.pack(">I", len(b)) + b + b"\0" * (-len(b) % 4)

    fill = 9.9692099683868690e+36
    head = b"CDF\x02" + struct.pack(">I", 0)
    head += struct.pack(">II", 10, len(dims)) + b"".join(name(n) + struct.pack(">I", k) for n, k in dims)
    head += struct.pack(">II", 12, len(gattrs)) + b"".join(name(n) + struct.pack(">II", 6, 1) + struct.pack(">d", v)
                                                           for n, v in gattrs)
    var_fixed = [name(n) + struct.pack(">I", len(dd)) + b"".join(struct.pack(">I", k) for k in dd) +
                 struct.pack(">II", 12, 1) + name("_FillValue") + struct.pack(">II", 6, 1) + struct.pack(">d", fill)
                 for n, dd, _ in variables]
    size = len(head) + 8 + sum(len(v) + 4 + 4 + 8 for v in var_fixed)
    out = head + struct.pack(">II", 11, len(variables))
    begin = size
    blobs = []
    for (n, dd, arr), vf in zip(variables, var_fixed):
        a = np.where(np.isnan(arr), fill, arr).astype(">f8")
        out += vf + struct.pack(">II", 6, a.nbytes) + struct.pack(">Q", begin)
        begin += a.nbytes
        blobs.append(a.tobytes())
    assert len(out) == size
    with open(path, "wb") as f:
        f.write(out + b"".join(blobs))


def write_xml():
    def prior(path, names):
        with open(path, "w") as f:
            f.write('<?xml version="1.0" encoding="utf-8"?>\n<variableset>\n')
            for n in names:
                i = NAMES.index(n)
                f.write(f'  <variable name="{n}" distribution="uniform" lower="{float(LOWER[i])!r}" upper="{float(UPPER[i])!r}"/>\n')
            f.write("</variableset>\n")
    prior(os.path.join(HERE, "incucyte_prior.xml"), NAMES)
    prior(os.path.join(HERE, "incucyte_prior_e1.xml"), NAMES[:-1])
    for fn, df in (("incucyte_likelihood.xml", "incucyte_data.json"), ("incucyte_likelihood_nc.xml", "incucyte_data.nc"),
                   ("incucyte_likelihood_e1.xml", "incucyte_data_e1.json")):
        with open(os.path.join(HERE, fn), "w") as f:
            f.write(f'<bcm_likelihood type="incucyte_population" drug="{DRUG}" cell_line="{CELL_LINE}" data_file="{df}"/>\n')


def skeleton():
    data = {}
    for k, ex in enumerate(EXPERIMENTS):
        T = len(ex["time"])
        z3 = np.zeros((T, C_, R_)).tolist()
        z2 = np.zeros((T, R_)).tolist()
        data[f"{DRUG}.{CELL_LINE}.experiment{k + 1}"] = dict(
            time=ex["time"], drug_concentrations=CONCENTRATIONS, drug_confluence=z3, drug_apoptosis_marker=z3,
            positive_control_confluence=z2, positive_control_apoptosis_marker=z2, negative_control_confluence=z2,
            negative_control_apoptosis_marker=z2, cell_titer_blue_norm=[0.0] * C_, treatment_time=ex["treatment_time"],
            ctb_time=ex["ctb_time"], seeding_density=ex["seeding_density"])
    return data


def make_data(lib):
    rng = np.random.default_rng(SEED + 1)
    data = skeleton()
    logp, wells, ctb, steps, codes = Driver(lib, data, NAMES).eval(TRUE)
    assert np.all(codes == 0), codes
    sc, sm, sb = TRUE[0], TRUE[1], TRUE[2]
    for k, ex in enumerate(EXPERIMENTS):
        g = data[f"{DRUG}.{CELL_LINE}.experiment{k + 1}"]
        T = len(ex["time"])
        conf, mark = wells[k, 3, :T], wells[k, 4, :T]  # [T][11]
        noise = lambda s, shape: s * rng.standard_t(3, size=shape)  # noqa: E731
        g["drug_confluence"] = (conf[:, :9, None] + noise(sc, (T, 9, R_))).tolist()
        g["drug_apoptosis_marker"] = (mark[:, :9, None] + noise(sm, (T, 9, R_))).tolist()
        g["positive_control_confluence"] = (conf[:, 9, None] + noise(sc, (T, R_))).tolist()
        g["positive_control_apoptosis_marker"] = (mark[:, 9, None] + noise(sm, (T, R_))).tolist()
        g["negative_control_confluence"] = (conf[:, 10, None] + noise(sc, (T, R_))).tolist()
        g["negative_control_apoptosis_marker"] = (mark[:, 10, None] + noise(sm, (T, R_))).tolist()
        g["cell_titer_blue_norm"] = (ctb[k] + noise(sb, 9)).tolist()
    data[f"{DRUG}.{CELL_LINE}.experiment1"]["drug_confluence"][5][2][1] = None  # one NaN observation
    return data


def draws():
    rng = np.random.default_rng(SEED)
    X = LOWER + (UPPER - LOWER) * rng.random((NDRAWS, len(NAMES)))
    hand = hand_rows()
    return np.vstack([X] + [r for _, r in hand]), [lab for lab, _ in hand]


def rel_dev(a, b):
    """largest |a - b| / max(|b|, tiny) over the finite entries of b"""
    m = np.isfinite(b)
    if not m.any():
        return 0.0
    return float(np.max(np.abs(a[m] - b[m]) / np.maximum(np.abs(b[m]), 1e-300)))


def golden(libs, data):
    X, labels = draws()
    fma = Driver(libs["fma"], data, NAMES).eval_rows(X)
    nof = Driver(libs["nofma"], data, NAMES).eval_rows(X)
    fin_f, fin_n = np.isfinite(fma[0]), np.isfinite(nof[0])
    assert np.array_equal(fin_f, fin_n), "the two reference builds disagree on which rows are finite"
    assert fin_n[:NDRAWS].mean() >= 0.75, f"only {fin_n[:NDRAWS].mean():.2f} of the prior draws are finite"
    fin = fin_n
    dies = NDRAWS + labels.index("negative_control_dies")
    assert np.all(fma[2][dies] == 0.0) and np.all(nof[2][dies] == 0.0), "the negative control does not die out"
    tol = dict(tol_logp=float(np.max(np.abs(fma[0][fin] - nof[0][fin]))),
               tol_wells=np.array([rel_dev(fma[1][fin][:, :, a], nof[1][fin][:, :, a]) for a in range(5)]),
               tol_ctb=rel_dev(fma[2][fin], nof[2][fin]))
    return dict(x=X, labels=np.array(labels), names=np.array(NAMES), logp_fma=fma[0], logp_nofma=nof[0], wells=nof[1],
                ctb=nof[2], steps=nof[3], codes=nof[4], **tol)


def main():
    libs = build()
    if "--time" in sys.argv:
        data = json.load(open(os.path.join(HERE, "incucyte_data.json")))
        d = Driver(libs["fma"], data, NAMES)
        X, _ = draws()
        t0 = time.perf_counter()
        for x in X[:NDRAWS]:
            d.eval(x)
        dt = (time.perf_counter() - t0) / NDRAWS
        print(json.dumps({"reference_driver_ms_per_evaluation": dt * 1e3, "rows": NDRAWS, "build": "fma", "threads": 1}))
        return
    if "--check" in sys.argv:
        data = json.load(open(os.path.join(HERE, "incucyte_data.json")))
        g = golden(libs, data)
        old = np.load(os.path.join(HERE, "incucyte_golden.npz"))
        for k in ("x", "logp_fma", "logp_nofma", "wells", "ctb", "steps", "codes"):
            assert np.array_equal(g[k], old[k], equal_nan=True), k
        print("incucyte_golden.npz regenerates row for row")
        return
    data = make_data(libs["nofma"])
    with open(os.path.join(HERE, "incucyte_data.json"), "w") as f:
        json.dump(data, f)
    e1 = {k: v for k, v in data.items() if k.endswith("experiment1")}
    with open(os.path.join(HERE, "incucyte_data_e1.json"), "w") as f:
        json.dump(e1, f)
    data = json.load(open(os.path.join(HERE, "incucyte_data.json")))  # as the tests read it
    write_classic(os.path.join(HERE, "incucyte_data.nc"), data)
    write_xml()
    g = golden(libs, data)
    np.savez_compressed(os.path.join(HERE, "incucyte_golden.npz"), **g)
    fin = np.isfinite(g["logp_nofma"])
    print(f"rows {len(fin)}, finite {fin.sum()} (prior draws {fin[:NDRAWS].mean():.2f}); tol logp {g['tol_logp']:.3g}, "
          f"wells {g['tol_wells']}, ctb {g['tol_ctb']:.3g}; bit-identical logp between builds "
          f"{np.mean(g['logp_fma'][fin] == g['logp_nofma'][fin]):.2f}")
    for lab, lp, cd, st, cb in zip(g["labels"], g["logp_nofma"][NDRAWS:], g["codes"][NDRAWS:], g["steps"][NDRAWS:], g["ctb"][NDRAWS:]):
        print(f"  {lab}: logp {lp:.6g} codes {sorted(set(cd.ravel().tolist()))} max steps {st.max()} ctb0 {cb[0, 0]:.3g}")


if __name__ == "__main__":
    main()
