// The engine's error type and SE_CHECK, free of any HIP header so that host-only headers (gc_select.h) and their stand-alone
// checks can use them.
#pragma once
#include <stdexcept>
#include <string>

namespace se {

struct Error : std::runtime_error {
    using std::runtime_error::runtime_error;
};

#define SE_STR2(x) #x
#define SE_STR(x) SE_STR2(x)
#define SE_CHECK(cond, msg)                                                                 \
    do {                                                                                    \
        if (!(cond)) throw ::se::Error(std::string(__FILE__ ":" SE_STR(__LINE__) ": ") + (msg)); \
    } while (0)

}  // namespace se
