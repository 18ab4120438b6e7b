// LikelihoodCellCycleMarker.cpp -- see LikelihoodCellCycleMarker.h
#include "LikelihoodCellCycleMarker.h"

#include <cerrno>
#include <climits>
#include <cstdlib>
#include <fstream>

#include "CSVParser.h"
#include "log.h"

namespace bcm3 {

namespace {

bool file_exists(const std::string& p)
{
    std::ifstream f(p);
    return (bool)f;
}

}  // namespace

// LikelihoodCellCycleMarker::Initialize (LikelihoodCellCycleMarker.cpp:18-54)
bool LikelihoodCellCycleMarker::Initialize(std::shared_ptr<const VariableSet> vs, const XmlNode& likelihood_node,
                                           const OptionsMap& vm)
{
    varset = vs;
    if (varset->GetNumVariables() != BCM3HIP_CCM_NVARS) {
        LOGERROR("Variable set should contain exactly 10 variables but contains %zd variables.", varset->GetNumVariables());
        return false;
    }

    // ccm.track_ix (AddOptionsDescription, .cpp:92-97): an int, default 0
    const std::string ix_str = option_get(vm, "ccm.track_ix", "0");
    char* end = nullptr;
    errno = 0;
    const long ix = std::strtol(ix_str.c_str(), &end, 10);
    if (ix_str.empty() || end == ix_str.c_str() || *end != '\0' || errno != 0 || ix < INT_MIN || ix > INT_MAX) {
        LOGERROR("ccm.track_ix: could not read \"%s\"", ix_str.c_str());
        return false;
    }
    const int use_track_ix = (int)ix;

    std::string data_file;
    try {
        data_file = likelihood_node.get("data_file");
    } catch (XmlError& e) {
        LOGERROR("Error parsing likelihood file: %s", e.what.c_str());
        return false;
    }
    // relative paths are tried against the working directory, then the likelihood file's directory
    std::string path = data_file;
    if (!file_exists(path)) {
        const std::string alt = option_get(vm, "likelihood_dir", ".") + "/" + data_file;
        if (file_exists(alt)) path = alt;
    }
    CSVParser parser;
    if (!parser.Parse(path, "\t")) {
        LOGERROR("Failed to parse data file \"%s\"", data_file.c_str());
        return false;
    }
    // (the reference's message counts the columns, the frames of a track, where it tests the rows)
    if (use_track_ix < 0 || (size_t)use_track_ix >= parser.GetNumRows()) {
        LOGERROR("Track index %d is out of bounds for data file with %zd columns.", use_track_ix, parser.GetNumColumns());
        return false;
    }
    LOG("Using track index %d.", use_track_ix);
    track_ix = use_track_ix;
    data = parser.GetRow((size_t)use_track_ix);
    // a track without frames gives logp = 0 for every vector in the reference; the device context
    // needs one frame at least
    if (data.empty()) {
        LOGERROR("Track %d of data file \"%s\" has no frames", use_track_ix, data_file.c_str());
        return false;
    }

    if (!OpenDevice(vm)) return false;
    if (option_get(vm, "backend", "") == "none") return true;
    bcm3hip_ccm_model m{(int32_t)data.size(), data.data()};
    const int r = bcm3hip_open_cell_cycle_marker(device, &m, &ctx);
    if (r != 0) {
        LOGERROR("Opening the cell_cycle_marker GPU context failed: %s", bcm3hip_error_string(r));
        return false;
    }
    return true;
}

}  // namespace bcm3
