// encode_norm.cuh — fragment of the three epilogues of encode_kernel and encode_blocked_kernel, included textually
// (profiles/encode_fragments.md): the row norm of token row r from the four column groups' sums of squares.
//   expects: r, sN complete and published (a __syncthreads() behind the last encode_pool.cuh)
//   defines: ss, nrm = max(sqrt(ss), 1e-12)  (candle.rs:218-225)
//   barriers: none
const float ss = ((sN[r] + sN[128 + r]) + (sN[256 + r] + sN[384 + r])); // fixed order: reproducible
float nrm = sqrtf(ss);
nrm = nrm < 1e-12f ? 1e-12f : nrm;
