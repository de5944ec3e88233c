// Expected majority vote over random orderings of one pool per problem (scv_resample_prefix<TOK>): the two instantiations.
#include "scvote_resample.hip.h"
namespace scv {
ResampleFn pick_resample_kernel(bool tok) {
    return tok ? (ResampleFn)scv_resample_prefix<true> : (ResampleFn)scv_resample_prefix<false>;
}
}  // namespace scv
