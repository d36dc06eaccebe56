// codecs_internal.h -- the codec entry points that cross translation units inside the library: included by the file that defines each of them and by
// every file that calls one, so that a changed signature fails to compile instead of failing to link (or linking).
#pragma once
#include <cstdint>
#include <vector>

// ---- baseline JPEG on the host (jpeg.cpp, jpeg_enc.cpp); SF_OK or an sf error code
int jpeg_decode_rgb(const uint8_t* data, uint64_t n, uint8_t* dst, uint32_t expect_w, uint32_t expect_h);
// entropy decoding only: SfJpegLayout + block table + coefficient entries (jpeg_idct.h), what jpeg_gpu_reconstruct / jpeg_gpu_planes take
int jpeg_decode_coef(const uint8_t* data, uint64_t n, uint32_t expect_w, uint32_t expect_h, uint8_t* payload, uint64_t payload_capacity);
// headers parsed, byte stuffing stripped: SfJpegLayout + SfJpegHuffDesc + the entropy-coded segment (jpeg_huff.h), what jpeg_gpu_huffman takes
int jpeg_prepare_huff(const uint8_t* data, uint64_t n, uint32_t expect_w, uint32_t expect_h, uint8_t* payload, uint64_t payload_capacity);
int jpeg_encode_rgb(const uint8_t* rgb, uint32_t width, uint32_t height, int quality, int subsample, std::vector<uint8_t>& out);

// ---- the codecs on the device: for translation units compiled as HIP (and for the ThreadSanitizer build against tools/tsan/fake_hip, which says so itself)
#if defined(__HIPCC__) || defined(SF_FAKE_HIP_RUNTIME)
#include <hip/hip_runtime.h>
void inflate_gpu_warm();     // inflate_gpu.hip, jpeg_gpu.hip, jpeg_huff_gpu.hip: load the file's code object now
void jpeg_gpu_warm();
void jpeg_huff_gpu_warm();
bool inflate_gpu_takes(const uint8_t* z, uint64_t n);  // inflate_gpu.hip
int inflate_gpu_batch(hipStream_t stream, int n, const uint32_t* const* d_words, const uint32_t* nbytes, uint8_t* const* d_out, uint16_t* const* d_plan, uint32_t expect,
                      const int32_t* tags, int32_t* d_status);  // inflate_gpu.hip
int jpeg_gpu_huffman(hipStream_t stream, int n, const uint8_t* const* d_prepared, uint8_t* const* d_payload, const uint32_t* max_entries, const int32_t* tags,
                     int32_t* d_status);  // jpeg_huff_gpu.hip
int jpeg_gpu_planes(hipStream_t stream, int n, const uint8_t* const* d_payload, uint8_t* const* d_planes, uint32_t max_blocks);   // jpeg_gpu.hip
int jpeg_gpu_reconstruct(hipStream_t stream, int n, const uint8_t* const* d_payload, uint8_t* const* d_rgb, uint8_t* const* d_planes, uint32_t max_blocks,
                         uint32_t max_width, uint32_t max_height);  // jpeg_gpu.hip
#endif
