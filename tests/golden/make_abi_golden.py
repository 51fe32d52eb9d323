"""Regenerates tests/golden/reference_abi.json from the REFERENCE's cffi headers.

    python tests/golden/make_abi_golden.py <reference libgdf include directory, the one holding gdf/cffi/>

Records what tests/test_abi.py compares include/gdf/gdf.h against: the function names functions.h and io_functions.h
declare, a digest of every prototype of the five cffi headers after `gcc -E` (return and parameter types, see
test_abi.prototype_digest), and the gdf_column / gdf_context layout and enumerator table that test_abi's layout program
prints when compiled against them.  The JSON holds data only (names, digests, numbers).
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

import test_abi  # noqa: E402


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref_inc = os.path.abspath(sys.argv[1])
    out = {
        "source": "reference include/gdf/cffi/{types,convert_types,functions,io_types,io_functions}.h",
        "functions": sorted(test_abi.reference_function_names(os.path.join(ref_inc, "gdf", "cffi"))),
        "prototype_sha256": {k: test_abi.prototype_digest(ret, ps) for k, (ret, ps) in sorted(test_abi.reference_prototypes(ref_inc).items())},
        "layout": test_abi.layout_table(ref_inc, ref=True),
    }
    with open(os.path.join(HERE, "reference_abi.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote reference_abi.json: {len(out['functions'])} functions, {len(out['prototype_sha256'])} prototypes")


if __name__ == "__main__":
    main()
