// prompt_table.h -- what prompt.hip and prompt_memory.hip share: how a (segment, row) table entry becomes a pool row, and the
// pointer and grid helpers of their entry points.  The rule that an entry outside its segment counts as -1 lives here alone.
#ifndef ZIRA_PROMPT_TABLE_H_
#define ZIRA_PROMPT_TABLE_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "zira_prompt.h"

namespace prompt_table {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWavesPerBlock = kThreads / kWave;      // a wave owns one row of D floats

typedef float f4 __attribute__((ext_vector_type(4)));   // 16 bytes, 16-byte aligned

// the pool row that the table gives to position `pos`, or nullptr where the row stays: a negative entry, a segment
// >= n_segments, a row >= the segment's rows, a segment without data
__device__ __forceinline__ const float *pool_row_of(const int32_t *__restrict__ table, const zira_prompt_segment *__restrict__ segments,
                                                    int pos, int D, int n_segments)
{
    const int seg = table[2 * pos], row = table[2 * pos + 1];
    if (seg < 0 || seg >= n_segments || row < 0) return nullptr;
    const zira_prompt_segment s = segments[seg];
    if (row >= s.rows || s.param == nullptr) return nullptr;
    return static_cast<const float *>(s.param) + (size_t)row * D;
}

inline bool aligned16(const void *p) { return p != nullptr && ((uintptr_t)p & 15) == 0; }
inline bool aligned8(const void *p) { return p != nullptr && ((uintptr_t)p & 7) == 0; }
inline bool aligned4(const void *p) { return p != nullptr && ((uintptr_t)p & 3) == 0; }
inline unsigned blocks_of(long long units) { return (unsigned)((units + kWavesPerBlock - 1) / kWavesPerBlock); }

}  // namespace prompt_table

#endif  // ZIRA_PROMPT_TABLE_H_
