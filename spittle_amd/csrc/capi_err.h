// capi_err.h -- how the C-ABI files report an error: the message copied into a caller's buffer, and
// for the contexts that keep a last error (a member `err`) the status of an exception thrown below the
// boundary and the try / catch around an entry point's body.
#pragma once
#include <string.h>

#include <exception>
#include <new>
#include <string>

#include "../../include/spittle_hip.h"
#include "common.h"

namespace spt {

inline void set_err(char* buf, size_t len, const std::string& m) {
    if (buf && len) {
        strncpy(buf, m.c_str(), len - 1);
        buf[len - 1] = 0;
    }
}

// record m as the context's last error and return s
template <typename Ctx>
spt_status fail(Ctx* c, spt_status s, const std::string& m) {
    if (c) c->err = m;
    return s;
}

// the Moonshine and SenseVoice boundaries' status of an exception (capi_pk.cpp and capi_vad.cpp map theirs
// differently)
inline spt_status classify(const std::exception& e) {
    if (dynamic_cast<const HipError*>(&e)) return SPT_ERR_DEVICE;
    if (dynamic_cast<const std::bad_alloc*>(&e)) return SPT_ERR_OOM;
    if (std::string(e.what()).find("out of device memory") != std::string::npos) return SPT_ERR_OOM;
    return SPT_ERR_INVALID_ARG;
}

// body() -> spt_status; an exception becomes its status, with the message as ctx's last error
template <typename Ctx, typename F>
spt_status guarded(Ctx* ctx, F&& body) {
    try {
        return body();
    } catch (const std::exception& e) {
        return fail(ctx, classify(e), e.what());
    }
}

}  // namespace spt
