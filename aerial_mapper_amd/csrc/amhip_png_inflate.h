// amhip_png_inflate.h -- the PNG decoder's inflate walk (amhip_png_decode.hip: k_pngd_inflate) for
// the other reader of zlib streams, the GeoTIFF reader (amhip_tiff_decode.hip): one launch function,
// so that there is one walk in the library.
#ifndef AMHIP_PNG_INFLATE_H_
#define AMHIP_PNG_INFLATE_H_

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "amhip_png_decode_host.h"

namespace amhip {
namespace pngd {

// RFC 1951 on streams frames[first .. first + n), one wave each, asynchronous on `stream`: the bytes
// [stream_begin, stream_end) of `bytes` -> raw + raw_base, raw_len bytes (stores cover raw_len rounded
// up to 16), checked against `adler`; status[first + k] = a pngd::Status.  `bytes` and every
// stream_begin - 2 in it lie at multiples of 16 (the bit reader loads aligned words), raw_base too.
// Only stream_begin, stream_end, adler, raw_len and raw_base of a Frame are read.
void launch_inflate(hipStream_t stream, const uint8_t* bytes, const Frame* frames, size_t first, size_t n,
                    uint8_t* raw, uint32_t* status);

}  // namespace pngd
}  // namespace amhip

#endif  // AMHIP_PNG_INFLATE_H_
