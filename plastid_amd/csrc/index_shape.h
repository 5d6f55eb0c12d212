// The geometry of a binning index (SAM specification 5.1.1, 5.3), shared by the index kernels (index_kernels.hip.h), the
// host finish (bam_index.h) and the host reader (bam_stager.cpp): leaves of 2^min_shift positions, n_lvls levels of 8
// children below the root.  BAI is (14, 5); a CSI carries its own shape.  Plain C++; usable in device code under hipcc.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PC_SHAPE_FN __host__ __device__ __forceinline__
#else
#define PC_SHAPE_FN inline
#endif

namespace pcshape {

constexpr int kBaiShift = 14, kBaiLvls = 5;

// the first bin of level l (hts_bin_first)
PC_SHAPE_FN uint32_t level_first(int l) { return (uint32_t)((((uint64_t)1 << (3 * l)) - 1u) / 7u); }
// the bins of an index with n_lvls levels below the root; its pseudo-bin is bin_count + 1 (hts.c:1092, 1179)
PC_SHAPE_FN uint32_t bin_count(int n_lvls) { return level_first(n_lvls + 1); }

struct IndexShape {
    bool csi = false;
    int min_shift = kBaiShift, n_lvls = kBaiLvls;
    int64_t reach() const { return (int64_t)1 << (min_shift + 3 * n_lvls); }   // the coordinates the index can hold
    uint32_t n_bins() const { return bin_count(n_lvls); }
    uint32_t meta_bin() const { return bin_count(n_lvls) + 1u; }               // 37450 for a BAI
};

} // namespace pcshape
