// CSVParser.h -- bcm3::CSVParser (src/utils/CSVParser.h): a separated-value table of Reals with a
// header line of column names and, by default, a first column of row names.
#pragma once
#include <string>
#include <vector>

#include "Likelihood.h"

namespace bcm3 {

class CSVParser {
public:
    // src/utils/CSVParser.cpp:9-78. The first line is the header (with rownames its first token is
    // dropped); every later line is one row. A trailing '\r' is stripped, empty tokens are kept, "NA"
    // and "nan" in any letter case become NaN and everything else goes through atof (a numeric
    // prefix is parsed, anything else is 0). A file that cannot be opened or is empty, and a row
    // whose length differs from the header's, are logged errors.
    bool Parse(const std::string& filename, const char* sep, bool rownames = true);

    size_t GetNumRows() const { return Rows.size(); }
    size_t GetNumColumns() const { return ColumnNames.size(); }
    Real GetEntry(size_t row, size_t col) const { return Rows[row][col]; }
    const std::vector<Real>& GetRow(size_t row) const { return Rows[row]; }
    const std::string& GetColumnName(size_t i) const { return ColumnNames[i]; }
    const std::string& GetRowName(size_t i) const { return RowNames[i]; }

private:
    std::vector<std::string> ColumnNames, RowNames;
    std::vector<std::vector<Real>> Rows;
};

}  // namespace bcm3
