// keyed_lattice.h -- the argument checks that open every entry point on a 3-D lattice of int32 keys.  Host only.
#pragma once
#include "clift_dev.h"

// `what`: the entry point's name.  max_dim: the bound on every dimension, 0 for none.  max_keys: valid keys are 0 .. n_keys - 1 with n_keys in
// 1 .. max_keys; 0 for a lattice without a key table (clift_cc_label).  Returns 1 with the error set, else 0.
static inline int keyed_lattice_check(const char* what, int n0, int n1, int n2, int max_dim, int n_keys, int max_keys) {
    if (max_dim > 0)
        CLIFT_REQUIRE(n0 >= 1 && n1 >= 1 && n2 >= 1 && n0 <= max_dim && n1 <= max_dim && n2 <= max_dim,
                      "%s: lattice dimensions must be 1 .. %d (got %d x %d x %d)", what, max_dim, n0, n1, n2);
    CLIFT_REQUIRE(n0 >= 1 && n1 >= 1 && n2 >= 1, "%s: lattice dimensions must be positive (got %d x %d x %d)", what, n0, n1, n2);
    const long total = (long)n0 * n1 * n2;
    CLIFT_REQUIRE(total < CLIFT_ISO_LIMIT, "%s: %ld lattice points (%d x %d x %d), must be < 2^31", what, total, n0, n1, n2);
    if (max_keys > 0) CLIFT_REQUIRE(n_keys >= 1 && n_keys <= max_keys, "%s: n_keys must be 1 .. %d (got %d)", what, max_keys, n_keys);
    return 0;
}
