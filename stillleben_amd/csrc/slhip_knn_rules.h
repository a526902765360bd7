// slhip_knn_rules.h -- the rules of the point k-NN (slhip_point_knn.hip) as plain float32 C++ for host and device alike:
// k_point_knn and slhip_point_knn_host run the same functions, so every output agrees bit for bit, and tests/point_knn_ref.py
// restates them in NumPy.  Every operation is one rounded IEEE operation (the build passes -ffp-contract=off); only - * + and
// comparisons appear.  The parenthesisation is the contract (include/slhip.h "Point neighbours", DESIGN.md "Point neighbours").
//
// Nothing here is a new distance: dist2 and is_finite are those of the pose errors (slhip_pose_rules.h), the rule by which a
// point counts is ICP's (slhip_icp_rules.h rule 2).  What is new is the list: the first k candidates of a query in the total
// order (distance, index), kept sorted, built by a scan upwards over the references.  Because the order is total, the list does
// not depend on how the scan is cut into tiles, nor on the K >= k slots that hold it.
#pragma once

#include <math.h>
#include <stdint.h>

#include "slhip.h"
#include "slhip_pose_rules.h"      // dist2, is_finite

namespace slhip_knn {

using slhip_pose::dist2;
using slhip_pose::is_finite;

constexpr uint32_t BLOCK = SLHIP_KNN_BLOCK;      // the queries of a workgroup, one per lane
constexpr uint32_t TILE = SLHIP_KNN_TILE;        // the references of an LDS tile
constexpr int EMPTY = -1;                        // the index of a slot without a neighbour

// rule 1: point (x, y, z, w) counts (the rule of ICP)
SLHIP_HD bool counts(float x, float y, float z, float w) { return w != 0.0f && is_finite(x) && is_finite(y) && is_finite(z); }

// rule 3: the square the distances are compared with (+inf: no gate)
SLHIP_HD float gate2(float max_dist) { return max_dist * max_dist; }

// rule 3 for the distance alone: finite and inside the gate, the gate's own distance included
SLHIP_HD bool passes(float d, float g2) { return is_finite(d) && d <= g2; }

// rule 3: reference r at distance d is a candidate of query q.  `self` is q under skip_same and EMPTY without it: the decision
// is by index, never by coordinates (duplicated points are normal)
SLHIP_HD bool candidate(bool query_counts, bool ref_counts, float d, float g2, int r, int self)
{
    return query_counts && ref_counts && passes(d, g2) && r != self;
}

// rule 4: a candidate of the scan upwards enters the list when its distance lies under the list's last one, strictly; an empty
// slot holds +inf here (rule 5 turns it into NaN on the way out), so a list that is not full takes every candidate
SLHIP_HD bool enters(float d, float last) { return d < last; }

// a list before the scan
template <int K>
SLHIP_HD void clear(float (&d)[K], int (&r)[K])
{
#pragma unroll
    for (int j = 0; j < K; ++j) {
        d[j] = __builtin_inff();
        r[j] = EMPTY;
    }
}

// rule 4: (x, ri) with enters(x, d[K - 1]) goes behind every entry with d' <= x; the entries behind it move up by one and the
// last one leaves.  Static indices throughout: slot j takes slot j - 1 when that one lies behind x, else x when slot j itself
// lies behind x, else it stays.  Every slot reads the list as it was before the call (j runs downwards).
template <int K>
SLHIP_HD void insert(float (&d)[K], int (&r)[K], float x, int ri)
{
#pragma unroll
    for (int j = K - 1; j > 0; --j) {
        const bool up = d[j - 1] > x, here = d[j] > x;
        r[j] = up ? r[j - 1] : here ? ri : r[j];
        d[j] = up ? d[j - 1] : here ? x : d[j];
    }
    const bool here = d[0] > x;
    r[0] = here ? ri : r[0];
    d[0] = here ? x : d[0];
}

// the same on a list of k slots known at run time (the host twin's)
inline void insert_n(float* d, int* r, uint32_t k, float x, int ri)
{
    uint32_t j = k - 1u;
    for (; j > 0u && d[j - 1u] > x; --j) {
        d[j] = d[j - 1u];
        r[j] = r[j - 1u];
    }
    d[j] = x;
    r[j] = ri;
}

// rule 5: what a slot holds on the way out
SLHIP_HD float slot_dist2(float d, int r) { return r == EMPTY ? __builtin_nanf("") : d; }

}  // namespace slhip_knn
