// lab.h -- the ONLY place this library consults anything but its arguments.
//
// The library reads no environment variable: a stray GDF_* variable in a caller's environment must not change which
// algorithm a drop-in library runs.  What remains here are the PATH SELECTORS the parity tests need (the same join /
// group-by through two different code paths must give the same answer): forced(), and path / path_on / path_int on top
// of it.  A selector is set ONLY through the exported test hook gdf_amd_debug_force(name, value)
// (include/gdf/gdf_amd_ext.h, libgdf_testhook.so); without the hook every selector reads as unset.  There is no other
// switch: no experiment knob, no second build of these sources.
#pragma once
#include <cstdlib>

namespace gdf_amd {
namespace lab {

// plumbing.cpp: value set through gdf_amd_debug_force, or nullptr.  The returned pointer is an interned string that is
// never freed (the library itself never writes the registry).
const char *forced(const char *name);

static inline const char *path(const char *name) { return forced(name); }
static inline bool path_on(const char *name) { return path(name) != nullptr; }
static inline long long path_int(const char *name, long long dflt) { const char *v = path(name); return v ? atoll(v) : dflt; }

// plumbing.cpp: tell the test-hook library which route a call took (read back by gdf_amd_debug_noted).  Does nothing -- one pointer
// test -- in every process that has not loaded libgdf_testhook.so; the library never reads a note.
void note(const char *name, long long value);

}  // namespace lab
}  // namespace gdf_amd
