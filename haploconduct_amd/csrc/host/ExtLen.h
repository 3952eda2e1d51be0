// ExtLen.h — Edge::ext_len (src/Edge.h:220-275) on a flattened edge record and the geometry of its two reads, shared by
// the host mirror of removeTips (host_model.cpp) and the device kernels (hc_trans_kernels.hip).  Plain C++ that also
// compiles as device code; the arithmetic is the reference's as written.
#pragma once
#include <stdint.h>

#include "../../../include/hcedge.h"

#if defined(__HIPCC__)
#define HC_EXT_HD __host__ __device__
#else
#define HC_EXT_HD
#endif

namespace hc {

HC_EXT_HD inline unsigned int ext_clamp(int x) { return (unsigned int)(x > 0 ? x : 0); }  // std::max(int, 0) into unsigned

// forward: by how many bases read2 extends read1; otherwise the other way round
HC_EXT_HD inline unsigned int edge_ext_len(const hc_edge_rec& e, const hc_read_geom& r1, const hc_read_geom& r2, bool forward) {
    const bool type1 = r1.paired != 0, type2 = r2.paired != 0;
    if (!forward) {  // :266-273: pos1 or pos1 + pos2, an int converted to unsigned (a negative sum wraps)
        if (type1 && type2 && e.ord == '1') return (unsigned int)e.pos1;
        return (unsigned int)(e.pos1 + e.pos2);
    }
    const int read2_len = (int)(type2 ? r2.len1 + r2.len2 : r2.len1);  // Read::get_len (src/Read.h:203-212)
    if ((type1 && type2 && e.ord == '1') || (!type1 && !type2)) return ext_clamp(read2_len - e.len0);  // P-P or S-S
    // get_seq(1) / get_seq(2) of read2, in the order the orientation gives
    const int readlen1 = (int)(e.ori2 ? r2.len1 : r2.len2), readlen2 = (int)(e.ori2 ? r2.len2 : r2.len1);
    if (type1 && type2 && e.ord == '2') return ext_clamp(readlen1 - e.len1) + ext_clamp(readlen2 - e.pos2 - e.len2);  // unsigned sum
    if (!type1 && type2) {  // S-P
        const unsigned int a = ext_clamp(readlen1 - e.len1), b = ext_clamp(readlen2 - e.len2);
        return a > b ? a : b;
    }
    return ext_clamp(read2_len - e.pos2 - e.len2);  // P-S (and P-P with neither '1' nor '2')
}

}  // namespace hc
