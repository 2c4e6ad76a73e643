// cat_max.h -- the one definition of "the max of a category's token logits and where it sits", shared by catlogits.hip
// (token logits read from memory) and clslinear.hip (token logits formed on chip).
#ifndef ZIRA_CAT_MAX_H_
#define ZIRA_CAT_MAX_H_

#include <hip/hip_runtime.h>

// Tokens are offered in token order, starting from best = -inf, at = -1.  A token of the category joins only when its logit is
// STRICTLY greater: of equal logits the first in token order stays (torch.max's index, and where the backward sends the
// category's gradient), and a category whose tokens are all -inf -- or that has none -- keeps at = -1 and reads `for_fill`.
__device__ __forceinline__ void zira_cat_max_step(bool in_category, float v, int t, float &best, int &at)
{
    if (in_category && v > best) { best = v; at = t; }
}

__device__ __forceinline__ float zira_cat_max_value(float best, int at, float for_fill) { return at >= 0 ? best : for_fill; }

#endif  // ZIRA_CAT_MAX_H_
