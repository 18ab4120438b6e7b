// capi_internal.h -- the handle behind include/bcm3.h's bcm3_likelihood, shared by the C-ABI files.
#pragma once
#include <cstring>
#include <memory>
#include <string>

#include "Likelihood.h"
#include "log.h"

struct bcm3_likelihood {
    std::shared_ptr<bcm3::VariableSet> varset;
    std::shared_ptr<bcm3::Likelihood> ll;
};

namespace bcm3 {

// a config string into a fixed char field of a C-ABI struct; false (with an error) when it does not fit
inline bool CopyConfigString(char* dst, size_t cap, const std::string& src, const char* what)
{
    if (src.size() + 1 > cap) {
        LOGERROR("config: %s is longer than %zu characters", what, cap - 1);
        return false;
    }
    std::memcpy(dst, src.c_str(), src.size() + 1);
    return true;
}

}  // namespace bcm3
