// LikelihoodIncucyte.cpp -- see LikelihoodIncucyte.h
#include "LikelihoodIncucyte.h"

#include <cmath>
#include <fstream>
#include <limits>
#include <set>

#include "NetCDFClassic.h"
#include "json.h"
#include "log.h"

namespace bcm3 {

namespace {

bool file_exists(const std::string& p)
{
    std::ifstream f(p);
    return (bool)f;
}

// the size of an array along each dimension (rectangular: the first element's at every level)
std::vector<size_t> shape_of(const Json& a)
{
    std::vector<size_t> s;
    const Json* p = &a;
    while (p->type == Json::Array) {
        s.push_back(p->arr.size());
        if (p->arr.empty()) break;
        p = &p->arr[0];
    }
    return s;
}

bool flatten(const Json& a, const std::vector<size_t>& shape, size_t level, std::vector<Real>& out)
{
    if (level == shape.size()) {
        if (a.type == Json::Array || a.type == Json::Object) return false;
        out.push_back(a.as_double());
        return true;
    }
    if (a.type != Json::Array || a.arr.size() != shape[level]) return false;
    for (auto& e : a.arr)
        if (!flatten(e, shape, level + 1, out)) return false;
    return true;
}

}  // namespace

// LikelihoodIncucytePopulation::Initialize (LikelihoodIncucytePopulation.cpp:31-145)
bool LikelihoodIncucytePopulation::Initialize(std::shared_ptr<const VariableSet> vs, const XmlNode& likelihood_node,
                                              const OptionsMap& vm)
{
    varset = vs;
    try {
        drug_name = likelihood_node.get("drug");
        cell_line = likelihood_node.get("cell_line");
    } catch (XmlError& e) {
        LOGERROR("Error parsing likelihood file: %s", e.what.c_str());
        return false;
    }
    // the reference's fixed file name unless a data_file attribute names another; relative paths are
    // tried against the working directory, then the likelihood file's directory
    const std::string data_file = likelihood_node.has_attr("data_file") ? likelihood_node.get("data_file") : "drug_response_data.nc";
    std::string path = data_file;
    if (!file_exists(path)) {
        const std::string alt = option_get(vm, "likelihood_dir", ".") + "/" + data_file;
        if (file_exists(alt)) path = alt;
    }
    Json data;
    try {
        data = LoadDataFile(path);
        UnwrapDataVariables(data);
    } catch (JsonError& e) {
        LOGERROR("Failed to open data file %s: %s", data_file.c_str(), e.what.c_str());
        return false;
    }

    // GetSubgroups(<drug>/<cell_line>): the groups directly below it ('.' separates the levels in the
    // flattened formats, '/' in netCDF-4 group paths)
    std::set<std::string> subgroups;
    for (const char sep : {'.', '/'}) {
        const std::string base = drug_name + sep + cell_line + sep;
        for (auto& g : data.obj)
            if (g.first.compare(0, base.size(), base) == 0 && g.first.size() > base.size())
                subgroups.insert(g.first.substr(base.size(), g.first.find_first_of("./", base.size()) - base.size()));
    }
    const size_t num_experiments = subgroups.size();
    if (num_experiments == 0) {
        LOGERROR("Could not find any experiments for drug \"%s\" and cell line \"%s\" in the data file", drug_name.c_str(),
                 cell_line.c_str());
        return false;
    }

    bool result = true;
    experiments.resize(num_experiments);
    for (size_t ei = 0; ei < num_experiments; ei++) {
        Experiment& e = experiments[ei];
        const std::string leaf = "experiment" + std::to_string(ei + 1);
        const Json* g = data.find(drug_name + "." + cell_line + "." + leaf);
        if (!g) g = data.find(drug_name + "/" + cell_line + "/" + leaf);
        if (!g) {
            LOGERROR("Group \"%s/%s/%s\" not found in %s (%zu experiment groups, which are numbered from 1)",
                     drug_name.c_str(), cell_line.c_str(), leaf.c_str(), path.c_str(), num_experiments);
            return false;
        }
        auto array = [&](const std::string& name, const std::vector<size_t>* want, std::vector<Real>& out,
                         std::vector<size_t>* got) -> bool {
            const Json* v = g->find(name);
            if (!v) {
                LOGERROR("Variable \"%s\" not found in group \"%s\"", name.c_str(), leaf.c_str());
                return false;
            }
            const std::vector<size_t> shape = shape_of(*v);
            if (want && shape != *want) {
                LOGERROR("Variable \"%s\" of group \"%s\" does not have the dimensions of the group", name.c_str(), leaf.c_str());
                return false;
            }
            out.clear();
            if (!flatten(*v, shape, 0, out)) {
                LOGERROR("Variable \"%s\" of group \"%s\" is not a rectangular numeric array", name.c_str(), leaf.c_str());
                return false;
            }
            if (got) *got = shape;
            return true;
        };
        auto attribute = [&](const std::string& name, Real& out) -> bool {
            const Json* v = g->find(name);
            if (v && v->type == Json::Array && v->arr.size() == 1) v = &v->arr[0];
            if (!v || (v->type != Json::Number && v->type != Json::Null)) {
                LOGERROR("Attribute \"%s\" not found in group \"%s\"", name.c_str(), leaf.c_str());
                return false;
            }
            out = v->as_double();
            return true;
        };
        // dimensions time / drug_concentrations from their coordinate variables, replicates from the
        // drug wells' last dimension
        std::vector<size_t> st, sc, sd;
        std::vector<Real> conc;
        if (!array("time", nullptr, e.time, &st) || !array("drug_concentrations", nullptr, conc, &sc) ||
            !array("drug_confluence", nullptr, e.drug_confluence, &sd))
            return false;
        if (st.size() != 1 || sc.size() != 1 || sd.size() != 3 || sd[0] != st[0] || sd[1] != sc[0]) {
            LOGERROR("Group \"%s\": time and drug_concentrations should be vectors and drug_confluence "
                     "[time][drug_concentrations][replicates]", leaf.c_str());
            return false;
        }
        e.num_timepoints = st[0];
        e.num_concentrations = sc[0];
        e.num_replicates = sd[2];
        if (e.num_timepoints == 0) {
            LOGERROR("Group \"%s\" has no time points", leaf.c_str());
            return false;
        }
        // the reference's loops run over exactly 9 concentrations and 4 replicates whatever the data
        // holds; with fewer it reads past the end of its arrays
        if (e.num_concentrations < BCM3HIP_INCUCYTE_CONCENTRATIONS) {
            LOGERROR("Group \"%s\" has %zu drug concentrations; the drug-effect curve is evaluated at exactly %d, so at "
                     "least %d are needed", leaf.c_str(), e.num_concentrations, (int)BCM3HIP_INCUCYTE_CONCENTRATIONS,
                     (int)BCM3HIP_INCUCYTE_CONCENTRATIONS);
            return false;
        }
        if (e.num_replicates < BCM3HIP_INCUCYTE_REPLICATES) {
            LOGERROR("Group \"%s\" has %zu replicates; the likelihood reads exactly %d per well, so at least %d are needed",
                     leaf.c_str(), e.num_replicates, (int)BCM3HIP_INCUCYTE_REPLICATES, (int)BCM3HIP_INCUCYTE_REPLICATES);
            return false;
        }
        e.log10_concentration.resize(conc.size());
        for (size_t ci = 0; ci < conc.size(); ci++) e.log10_concentration[ci] = log10(conc[ci]);
        const std::vector<size_t> well = {e.num_timepoints, e.num_concentrations, e.num_replicates};
        const std::vector<size_t> control = {e.num_timepoints, e.num_replicates};
        const std::vector<size_t> per_conc = {e.num_concentrations};
        result &= array("drug_apoptosis_marker", &well, e.drug_marker, nullptr);
        result &= array("positive_control_confluence", &control, e.pao_confluence, nullptr);
        result &= array("positive_control_apoptosis_marker", &control, e.pao_marker, nullptr);
        result &= array("negative_control_confluence", &control, e.neg_confluence, nullptr);
        result &= array("negative_control_apoptosis_marker", &control, e.neg_marker, nullptr);
        result &= array("cell_titer_blue_norm", &per_conc, e.ctb, nullptr);
        result &= attribute("treatment_time", e.treatment_time);
        result &= attribute("ctb_time", e.ctb_time);
        result &= attribute("seeding_density", e.seeding_density);
        if (!result) return false;
    }

    // every variable EvaluateLogProbability / SimulateWell look up by name on the S-curve path; the
    // reference indexes the value vector with GetVariableIndex's "not found" (out of range) otherwise
    const size_t absent = std::numeric_limits<size_t>::max();
    for (int k = 0; k < BCM3HIP_INC_NVARS; k++) {
        const std::string name = bcm3hip_incucyte_variable_name(k);
        const size_t i = varset->GetVariableIndex(name, false);
        if (i == absent) {
            LOGERROR("incucyte_population needs the variable \"%s\", which is not in the prior", name.c_str());
            return false;
        }
        model.variables.ix[k] = (int32_t)i;
    }
    for (size_t ei = 0; ei < num_experiments; ei++) {
        const std::string name = "seeding_density_deviation_" + std::to_string(ei + 1);
        const size_t i = varset->GetVariableIndex(name, false);
        if (i == absent) {
            LOGERROR("incucyte_population needs the variable \"%s\" (one per experiment), which is not in the prior",
                     name.c_str());
            return false;
        }
        experiments[ei].seeding_density_deviation_ix = (int32_t)i;
    }

    dev_experiments.resize(num_experiments);
    for (size_t ei = 0; ei < num_experiments; ei++) {
        const Experiment& e = experiments[ei];
        bcm3hip_incucyte_experiment& x = dev_experiments[ei];
        x.T = (int32_t)e.num_timepoints;
        x.C = (int32_t)e.num_concentrations;
        x.R = (int32_t)e.num_replicates;
        x.seeding_density_deviation_ix = e.seeding_density_deviation_ix;
        x.treatment_time = e.treatment_time;
        x.seeding_density = e.seeding_density;
        x.time = e.time.data();
        x.log10_concentration = e.log10_concentration.data();
        x.drug_confluence = e.drug_confluence.data();
        x.drug_marker = e.drug_marker.data();
        x.pao_confluence = e.pao_confluence.data();
        x.pao_marker = e.pao_marker.data();
        x.neg_confluence = e.neg_confluence.data();
        x.neg_marker = e.neg_marker.data();
        x.ctb = e.ctb.data();
    }
    model.d = (int32_t)varset->GetNumVariables();
    model.E = (int32_t)num_experiments;
    model.experiments = dev_experiments.data();

    if (!OpenDevice(vm)) return false;
    if (option_get(vm, "backend", "") == "none") return true;
    int r = bcm3hip_open_incucyte(device, &model, &ctx);
    if (r != 0) {
        LOGERROR("bcm3hip_open_incucyte failed: %s", bcm3hip_error_string(r));
        return false;
    }
    return true;
}

}  // namespace bcm3
