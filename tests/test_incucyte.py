"""incucyte_population on the host: loading (backend=none), validation messages, LogPdfTnu3, the
C-ABI declarations, and -- where the reference driver has been built -- the fixture's regeneration."""
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

from bcm3_amd import _hip  # noqa: E402
from bcm3_amd.likelihood import Likelihood  # noqa: E402

PRIOR = os.path.join(G, "incucyte_prior.xml")
ARRAYS = ("time", "log10_concentration", "drug_confluence", "drug_marker", "pao_confluence", "pao_marker",
          "neg_confluence", "neg_marker", "ctb")


def load(xml, prior=PRIOR):
    return Likelihood(os.path.join(G, xml) if not os.path.isabs(xml) else xml, prior, options="backend=none")


def test_loads_from_json_and_classic_with_identical_arrays():
    a = load("incucyte_likelihood.xml").incucyte_model()
    b = load("incucyte_likelihood_nc.xml").incucyte_model()
    assert a["E"] == b["E"] == 2 and a["d"] == 33
    assert a["variables"] == b["variables"] and len(a["variables"]) == _hip.INC_NVARS
    for ea, eb in zip(a["experiments"], b["experiments"]):
        for k in ("T", "C", "R", "seeding_density_deviation_ix", "treatment_time", "seeding_density"):
            assert ea[k] == eb[k], k
        for k in ARRAYS:
            assert np.array_equal(ea[k], eb[k], equal_nan=True), k
    e0, e1 = a["experiments"]
    assert (e0["T"], e0["C"], e0["R"]) == (12, 9, 4) and e1["T"] == 11
    assert e0["time"][0] == 0.0 and e0["treatment_time"] in e0["time"]
    assert np.isnan(e0["drug_confluence"]).sum() == 1
    raw = json.load(open(os.path.join(G, "incucyte_data.json")))["drugA.lineX.experiment1"]
    assert np.array_equal(e0["log10_concentration"], np.log10(np.array(raw["drug_concentrations"])))
    names = Likelihood(os.path.join(G, "incucyte_likelihood.xml"), PRIOR, options="backend=none").variable_names
    assert names[e1["seeding_density_deviation_ix"]] == "seeding_density_deviation_2"


def test_experiment_count_follows_the_subgroups():
    m = load("incucyte_likelihood_e1.xml", os.path.join(G, "incucyte_prior_e1.xml")).incucyte_model()
    assert m["E"] == 1 and m["d"] == 32


def _variant(tmp_path, edit_data=None, drop_variable=None, drug="drugA", cell_line="lineX"):
    data = json.load(open(os.path.join(G, "incucyte_data.json")))
    if edit_data:
        edit_data(data)
    json.dump(data, open(tmp_path / "data.json", "w"))
    xml = tmp_path / "likelihood.xml"
    xml.write_text(f'<bcm_likelihood type="incucyte_population" drug="{drug}" cell_line="{cell_line}" data_file="data.json"/>\n')
    prior = tmp_path / "prior.xml"
    text = open(PRIOR).read()
    if drop_variable:
        text = "\n".join(line for line in text.splitlines() if f'name="{drop_variable}"' not in line)
    prior.write_text(text)
    return str(xml), str(prior)


def _fails(xml, prior, pattern):
    with pytest.raises(RuntimeError) as e:
        Likelihood(xml, prior, options="backend=none")
    assert re.search(pattern, str(e.value)), str(e.value)


@pytest.mark.parametrize("name", ["sigma_ctb", "pao_effect_time", "contact_inhibition_apoptosis_rate",
                                  "seeding_density_deviation_2"])
def test_missing_required_variable_is_named(tmp_path, name):
    _fails(*_variant(tmp_path, drop_variable=name), f'needs the variable "{name}"')


def test_fewer_than_nine_concentrations_refused(tmp_path):
    def cut(data):
        g = data["drugA.lineX.experiment2"]
        g["drug_concentrations"] = g["drug_concentrations"][:8]
        g["cell_titer_blue_norm"] = g["cell_titer_blue_norm"][:8]
        for k in ("drug_confluence", "drug_apoptosis_marker"):
            g[k] = [row[:8] for row in g[k]]
    _fails(*_variant(tmp_path, cut), r"8 drug concentrations.*exactly 9")


def test_fewer_than_four_replicates_refused(tmp_path):
    def cut(data):
        g = data["drugA.lineX.experiment1"]
        for k in ("drug_confluence", "drug_apoptosis_marker"):
            g[k] = [[c[:3] for c in row] for row in g[k]]
        for k in ("positive_control_confluence", "positive_control_apoptosis_marker", "negative_control_confluence",
                  "negative_control_apoptosis_marker"):
            g[k] = [row[:3] for row in g[k]]
    _fails(*_variant(tmp_path, cut), r"3 replicates.*exactly 4")


def test_unknown_drug_or_cell_line(tmp_path):
    _fails(*_variant(tmp_path, drug="drugB"), r'Could not find any experiments for drug "drugB" and cell line "lineX"')
    _fails(*_variant(tmp_path, cell_line="lineY"), r'Could not find any experiments for drug "drugA" and cell line "lineY"')


def test_log_pdf_tnu3_host_side():
    rng = np.random.default_rng(3)
    for x, mu, s in zip(rng.normal(0, 5, 200), rng.normal(0, 5, 200), rng.uniform(0.05, 4, 200)):
        xn = (x - mu) / s
        want = -1.0008888496235098 - 2.0 * np.log1p(0.333333333333333333 * xn * xn) - np.log(s)
        got = _hip.log_pdf_tnu3(x, mu, s)
        assert abs(got - want) <= 4 * np.finfo(float).eps * max(1.0, abs(want)), (x, mu, s)
    # the density integrates to one: the constant is log(Gamma(2) / (sqrt(3 pi) Gamma(3/2)))
    assert abs(-1.0008888496235098 - (math.lgamma(2.0) - math.lgamma(1.5) - 0.5 * math.log(3 * math.pi))) < 1e-15
    assert _hip.log_pdf_tnu3(float("nan"), 1.0, 2.0) == 0.0  # skip_na
    assert math.isnan(_hip.log_pdf_tnu3(1.0, float("nan"), 2.0))


def test_new_symbols_declared():
    hip = open(os.path.join(ROOT, "include", "bcm3hip.h")).read()
    for s in ("bcm3hip_open_incucyte", "bcm3hip_eval_batch_incucyte_detail", "bcm3hip_incucyte_variable_name",
              "bcm3hip_log_pdf_tnu3", "bcm3hip_incucyte_model", "bcm3hip_incucyte_experiment"):
        assert re.search(rf"\b{s}\b", hip), s
    host = open(os.path.join(ROOT, "include", "bcm3.h")).read()
    for s in ("bcm3_likelihood_incucyte_model", "bcm3_likelihood_incucyte_detail"):
        assert re.search(rf"\b{s}\(", host) and hasattr(__import__("bcm3_amd.likelihood").likelihood.lib(), s), s
    assert _hip.incucyte_variable_names()[:3] == ["sigma_confluence", "sigma_apoptosis_marker", "sigma_ctb"]
    assert _hip.lib().bcm3hip_incucyte_variable_name(_hip.INC_NVARS) is None


def test_fixture_conditions():
    g = np.load(os.path.join(G, "incucyte_golden.npz"))
    fin = np.isfinite(g["logp_nofma"])
    assert np.array_equal(fin, np.isfinite(g["logp_fma"]))
    assert fin[:64].mean() >= 0.75
    lab = list(g["labels"])
    codes = g["codes"][64:]
    assert -22 in codes[lab.index("stop_time_before_start")] and not fin[64 + lab.index("stop_time_before_start")]
    assert (codes[lab.index("history_exhausted")] == _hip.INC_HISTORY_FULL).any()
    assert np.all(g["ctb"][64 + lab.index("negative_control_dies")] == 0.0)


def test_fixture_regenerates_row_for_row():
    drv = os.path.join(ROOT, "oracle", "_ref", "incucyte", "libincucyteref_nofma.so")
    if not os.path.exists(drv) or not os.path.isdir(os.path.join(os.environ.get("REF", "/root/reference"), "dependencies", "cvode-5.3.0")):
        pytest.skip("the reference driver has not been built here (tests/golden/make_incucyte_fixtures.py)")
    r = subprocess.run([sys.executable, os.path.join(G, "make_incucyte_fixtures.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
