// The zlib encoder on the GPU, host side (revision 20): pc_deflate_zlib / pc_deflate_zlib_mode and pc_huffman_lengths of
// include/plastid_counts.h, the twins of pc_inflate_zlib.  The inputs cross PCIe once; k_zlib_deflate (deflate_kernels.hip.h) turns each into a stream in its
// slot of len + 16 bytes; the sizes, their exclusive sum and k_deflate_compact make one contiguous buffer, which is read
// back with the offsets and sizes.  The bytes are those of pcdeflate::encode (deflate_host.h).  From slot offsets to
// compacted streams the work is zlib_encode_stage over a ZlibEncodeStage, which the bigWig writer uses for its data
// sections and for its zoom blocks (bigwig_writer.hip.h); nothing else calls queue_zlib_deflate.
// Part of the one translation unit of plastid_counts.hip (behind bigwig_decoder.hip.h; the plumbing is device_util.hip.h).
#include "deflate_kernels.hip.h"

namespace {

// n inputs in HBM -> their streams, compacted into d_out (room for the sum of len + 11), on `st`.  d_slot_off: the
// exclusive sum of len + 16; d_len / d_off: n sizes and offsets of the streams; d_fell_back: how far every stream's block fell back from the mode's own codes
// (its BTYPE is mode - steps); mode: pcdeflate::kFixed or kDynamic; encoded (optional): recorded between the encoder and the compaction.
int queue_zlib_deflate(hipStream_t st, const uint8_t *d_image, const int64_t *d_in_off, const int64_t *d_in_len, const uint64_t *d_slot_off, int64_t n,
                       uint8_t *d_slots, unsigned long long *d_len, unsigned long long *d_off, uint32_t *d_fell_back, DevBuf<uint8_t> &d_tmp, uint8_t *d_out, uint32_t mode, hipEvent_t encoded = nullptr) {
    if (n == 0) return PC_OK;
    if (mode == pcdeflate::kDynamic)
        hipLaunchKernelGGL(pcdeflate::k_zlib_deflate<pcdeflate::kDynamic>, dim3((unsigned)n), dim3(pcdeflate::kDefWG), 0, st, d_image, d_in_off, d_in_len, d_slot_off, n, d_slots,
                           d_len, d_fell_back);
    else
        hipLaunchKernelGGL(pcdeflate::k_zlib_deflate<pcdeflate::kFixed>, dim3((unsigned)n), dim3(pcdeflate::kDefWG), 0, st, d_image, d_in_off, d_in_len, d_slot_off, n, d_slots,
                           d_len, d_fell_back);
    HIP_TRY(hipGetLastError());
    if (encoded) HIP_TRY(hipEventRecord(encoded, st));
    PC_TRY(cub_run(d_tmp, [&](void *tmp, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(tmp, b, d_len, d_off, (int)n, st); }));
    hipLaunchKernelGGL(pcdeflate::k_deflate_compact, dim3((unsigned)n), dim3(256), 0, st, (const uint8_t *)d_slots, d_slot_off, (const unsigned long long *)d_len,
                       (const unsigned long long *)d_off, n, d_out);
    HIP_TRY(hipGetLastError());
    return PC_OK;
}

// The encode stage: what turns n raw blocks in HBM into their streams, back to back.
struct ZlibEncodeStage {
    DevBuf<int64_t> d_in;                  // the offsets, then the lengths of the raw blocks: the caller's to fill
    DevBuf<uint64_t> d_slot_off;
    DevBuf<uint8_t> d_slots, d_out;        // every block's stream in its slot; the streams compacted
    DevBuf<unsigned long long> d_res;      // the sizes, then the offsets of the streams
    DevBuf<uint32_t> d_stored;             // how far every stream's block fell back
};

// The n blocks that z.d_in describes inside d_raw, block b of raw_size(b) bytes, through the encoder and the compaction
// on `st`, which has drained when this returns.  encoded / compacted (optional): recorded behind the encoder and behind
// the compaction.
template <typename RawSize>
int zlib_encode_stage(hipStream_t st, const uint8_t *d_raw, int64_t n, RawSize raw_size, uint32_t mode, DevBuf<uint8_t> &d_tmp, ZlibEncodeStage &z,
                      hipEvent_t encoded = nullptr, hipEvent_t compacted = nullptr) {
    std::vector<uint64_t> slot_off((size_t)n);
    uint64_t slots = 0, raw = 0;
    for (int64_t b = 0; b < n; ++b) { slot_off[(size_t)b] = slots; raw += raw_size(b); slots += raw_size(b) + pcdeflate::kSlotPad; }
    int rc = PC_OK;
    room(rc, z.d_slots, (size_t)slots + 64); room(rc, z.d_out, (size_t)(raw + (uint64_t)pcdeflate::kStreamOverhead * (uint64_t)n) + 64);
    room(rc, z.d_res, 2 * (size_t)n); room(rc, z.d_stored, (size_t)n);
    if (rc != PC_OK) return rc;
    PC_TRY(z.d_slot_off.upload(slot_off, st));
    PC_TRY(queue_zlib_deflate(st, d_raw, z.d_in.p, z.d_in.p + n, z.d_slot_off.p, n, z.d_slots.p, z.d_res.p, z.d_res.p + n, z.d_stored.p, d_tmp, z.d_out.p, mode, encoded));
    if (compacted) HIP_TRY(hipEventRecord(compacted, st));
    HIP_TRY(hipStreamSynchronize(st));   // (slot_off goes out of scope)
    return PC_OK;
}

}   // namespace

extern "C" {

int pc_deflate_zlib_mode(pc_engine *e, const void *image, int64_t n, const int64_t *off, const int64_t *len, void *out, int64_t out_capacity, int64_t *out_off,
                         int64_t *out_len, int mode) {
    if (mode != (int)pcdeflate::kFixed && mode != (int)pcdeflate::kDynamic) return fail(PC_ERR_ARG, "pc_deflate_zlib: mode %d is neither 1 (fixed) nor 2 (dynamic)", mode);
    if (!e || n < 0 || n >= ((int64_t)1 << 31) || out_capacity < 0 || (n > 0 && (!off || !len || !out || !out_off || !out_len)))
        return fail(PC_ERR_ARG, "pc_deflate_zlib: bad arguments");
    if (n == 0) return PC_OK;
    int64_t image_bytes = 0, need = 0;
    for (int64_t k = 0; k < n; ++k) {
        if (off[k] < 0 || len[k] < 0 || len[k] > (int64_t)pcdeflate::kMaxInput)
            return fail(PC_ERR_ARG, "pc_deflate_zlib: input %lld lies below 0 or holds more than %u bytes", (long long)k, pcdeflate::kMaxInput);
        if (len[k] > 0) image_bytes = std::max(image_bytes, off[k] + len[k]);
        need += len[k] + (int64_t)pcdeflate::kStreamOverhead;
    }
    if (image_bytes > 0 && !image) return fail(PC_ERR_ARG, "pc_deflate_zlib: bad arguments");
    if (out_capacity < need) return fail(PC_ERR_ARG, "pc_deflate_zlib: out_capacity %lld below the %lld bytes the streams may take", (long long)out_capacity, (long long)need);
    HIP_TRY(hipSetDevice(e->device));
    PoolScope pool_scope(&e->pool);
    hipStream_t st = e->stream;
    DevBuf<uint8_t> d_image, d_tmp;
    ZlibEncodeStage z;
    std::vector<int64_t> h_in(2 * (size_t)n);    // the offsets, then the lengths
    std::vector<unsigned long long> h_res(2 * (size_t)n);
    memcpy(h_in.data(), off, (size_t)n * 8); memcpy(h_in.data() + n, len, (size_t)n * 8);
    DrainOnExit drained{st};
    int rc = PC_OK;
    room(rc, d_image, (size_t)image_bytes + 64); room(rc, z.d_in, 2 * (size_t)n);
    if (rc != PC_OK) return rc;
    if (image_bytes > 0) HIP_TRY(hipMemcpyAsync(d_image.p, image, (size_t)image_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(z.d_in.p, h_in.data(), h_in.size() * 8, hipMemcpyHostToDevice, st));
    PC_TRY(zlib_encode_stage(st, d_image.p, n, [len](int64_t k) { return (uint64_t)len[k]; }, (uint32_t)mode, d_tmp, z));
    HIP_TRY(hipMemcpyAsync(h_res.data(), z.d_res.p, h_res.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t total = (int64_t)(h_res[(size_t)(2 * n - 1)] + h_res[(size_t)(n - 1)]);
    if (total > need) { drained.armed = false; return fail(PC_ERR_STATE, "pc_deflate_zlib: the streams hold %lld bytes, more than %lld", (long long)total, (long long)need); }
    HIP_TRY(hipMemcpyAsync(out, z.d_out.p, (size_t)total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    drained.armed = false;
    for (int64_t k = 0; k < n; ++k) { out_len[k] = (int64_t)h_res[(size_t)k]; out_off[k] = (int64_t)h_res[(size_t)(n + k)]; }
    return PC_OK;
}

int pc_deflate_zlib(pc_engine *e, const void *image, int64_t n, const int64_t *off, const int64_t *len, void *out, int64_t out_capacity, int64_t *out_off, int64_t *out_len) {
    return pc_deflate_zlib_mode(e, image, n, off, len, out, out_capacity, out_off, out_len, (int)pcdeflate::kFixed);
}

int pc_huffman_lengths(pc_engine *e, const uint32_t *counts, int64_t n, int limit, uint8_t *lengths_out) {
    if (!e || !counts || !lengths_out) return fail(PC_ERR_ARG, "pc_huffman_lengths: bad arguments");
    if (n < 2 || n > (int64_t)pcdeflate::kLitSyms || limit < 1 || limit > 15 || ((int64_t)1 << limit) < n)
        return fail(PC_ERR_ARG, "pc_huffman_lengths: %lld symbols under limit %d (2 .. 286 symbols, limit 1 .. 15, 2^limit >= symbols)", (long long)n, limit);
    uint64_t sum = 0;
    for (int64_t s = 0; s < n; ++s) sum += counts[s];
    if (sum >= ((uint64_t)1 << 32)) return fail(PC_ERR_ARG, "pc_huffman_lengths: the counts add up to 2^32 or more");
    HIP_TRY(hipSetDevice(e->device));
    PoolScope pool_scope(&e->pool);
    hipStream_t st = e->stream;
    DevBuf<uint32_t> d_counts;
    DevBuf<uint8_t> d_lengths;
    DrainOnExit drained{st};
    int rc = PC_OK;
    room(rc, d_counts, (size_t)n); room(rc, d_lengths, (size_t)n);
    if (rc != PC_OK) return rc;
    HIP_TRY(hipMemcpyAsync(d_counts.p, counts, (size_t)n * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(pcdeflate::k_huffman_lengths, dim3(1), dim3(pcdeflate::kDefWG), 0, st, (const uint32_t *)d_counts.p, (uint32_t)n, (uint32_t)limit, d_lengths.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(lengths_out, d_lengths.p, (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    drained.armed = false;
    return PC_OK;
}

}   // extern "C"
