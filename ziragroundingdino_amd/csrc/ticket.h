// ticket.h -- the cross-block arrival protocol of the kernels whose last block (or wave) to arrive finishes the job: every block
// stores its part, RELEASES it, and draws an integer ticket; whoever draws the last one ACQUIRES and reads all the parts with
// plain loads.  No block ever waits for another.  Everything here is internal linkage (one copy per TU).
//
// What this pins: the fences are agent-scope (one device) and each is followed by `s_waitcnt vmcnt(0)`, so the part's stores
// have left the wave before the ticket is drawn and nothing is loaded before the fence has taken effect; the ticket word wraps
// to zero behind the last draw (atomicInc), so the next launch -- or a graph replay -- finds it as the first one did and
// nobody clears it.
#ifndef ZIRA_TICKET_H_
#define ZIRA_TICKET_H_

#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ void release_agent()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

__device__ __forceinline__ void acquire_agent()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// lane 0 draws a ticket of a word that wraps behind `last`; every lane learns whether it was the last one
__device__ __forceinline__ bool drew_last(unsigned *word, unsigned last, int lane)
{
    unsigned t = 0;
    if (lane == 0) t = atomicInc(word, last);
    return (unsigned)__builtin_amdgcn_readfirstlane((int)t) == last;
}

}  // namespace

#endif  // ZIRA_TICKET_H_
