// The error return every translation unit shares (the g++ ones too: nothing of HIP here).
#pragma once

// records msg as the calling thread's mosaic_last_error and returns code (defined in mosaic_hip.hip)
extern "C" int mosaic_tess_fail(int code, const char* msg);

// passes a non-zero rc of expr up to the caller
#define MOSAIC_RC(expr)      \
    do {                     \
        int _rc = (expr);    \
        if (_rc) return _rc; \
    } while (0)
