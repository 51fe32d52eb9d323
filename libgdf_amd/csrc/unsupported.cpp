// unsupported.cpp -- exported stub for the one reference entry point that is still out of scope (csv reading; SURVEY.md
// section 2).  The cffi binding resolves symbols lazily (python/libgdf_cffi/wrapper.py:13-34), so a caller only meets it
// when it actually calls it; it then gets GDF_UNSUPPORTED_METHOD instead of a missing-symbol crash.
#include "gdf/gdf.h"

extern "C" {

gdf_error read_csv(csv_read_arg *) { return GDF_UNSUPPORTED_METHOD; }

}  // extern "C"
