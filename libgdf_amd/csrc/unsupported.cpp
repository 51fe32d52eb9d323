// unsupported.cpp -- exported stubs for the two reference entry points that are still out of scope (csv reading and the
// CSR conversion).  The cffi binding resolves symbols lazily (python/libgdf_cffi/wrapper.py:13-34),
// so a caller only meets these when it actually calls one; it then gets GDF_UNSUPPORTED_METHOD instead of a
// missing-symbol crash.
#include "gdf/gdf.h"

extern "C" {

gdf_error read_csv(csv_read_arg *) { return GDF_UNSUPPORTED_METHOD; }
gdf_error gdf_to_csr(gdf_column **, int, csr_gdf *) { return GDF_UNSUPPORTED_METHOD; }

}  // extern "C"
