// CSVParser.cpp -- see CSVParser.h
#include "CSVParser.h"

#include <strings.h>

#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>

#include "log.h"

namespace bcm3 {

namespace {

// bcm3::tokenize (src/utils/Utils.cpp:7-25): split at any character of delims, empty tokens kept
// (also a trailing one); an empty string has no tokens
void tokenize(const std::string& str, std::vector<std::string>& tokens, const char* delims)
{
    tokens.clear();
    if (str.empty()) return;
    size_t start = 0;
    for (;;) {
        const size_t end = str.find_first_of(delims, start);
        if (end == std::string::npos) {
            tokens.push_back(str.substr(start));
            return;
        }
        tokens.push_back(str.substr(start, end - start));
        start = end + 1;
    }
}

void strip_cr(std::string& line)
{
    if (!line.empty() && line.back() == '\r') line.pop_back();
}

}  // namespace

bool CSVParser::Parse(const std::string& filename, const char* sep, bool rownames)
{
    ColumnNames.clear();
    RowNames.clear();
    Rows.clear();
    std::ifstream ifs(filename.c_str());
    if (!ifs.is_open()) {
        LOGERROR("Could not open file \"%s\" for reading", filename.c_str());
        return false;
    }
    std::string line;
    if (!std::getline(ifs, line)) {
        LOGERROR("Could not read from file \"%s\"", filename.c_str());
        return false;
    }
    strip_cr(line);
    tokenize(line, ColumnNames, sep);
    if (ColumnNames.empty()) {
        LOGERROR("CSV file \"%s\" has no header with column names", filename.c_str());
        return false;
    }
    if (rownames) ColumnNames.erase(ColumnNames.begin());

    const size_t expected = ColumnNames.size() + (rownames ? 1 : 0);
    std::vector<std::string> rowstr;
    for (size_t data_line = 0; std::getline(ifs, line); data_line++) {
        strip_cr(line);
        tokenize(line, rowstr, sep);
        if (rowstr.size() != expected) {
            LOGERROR("Inconsistent CSV data file \"%s\": found %zu instead of %zu data points at data line %zu",
                     filename.c_str(), rowstr.size(), ColumnNames.size(), data_line);
            return false;
        }
        RowNames.push_back(rownames ? rowstr[0] : std::to_string(data_line));
        std::vector<Real> row(ColumnNames.size());
        for (size_t i = 0; i < row.size(); i++) {
            const char* value = rowstr[i + (rownames ? 1 : 0)].c_str();
            if (strcasecmp(value, "NA") == 0 || strcasecmp(value, "nan") == 0)
                row[i] = std::numeric_limits<Real>::quiet_NaN();
            else
                row[i] = std::atof(value);
        }
        Rows.push_back(std::move(row));
    }
    return true;
}

}  // namespace bcm3
