// The best `keep` keys of a step, in order -- TEXT that code_search_kx8.hip and code_search_kx8_xtx.hip include inside their kernels
// at the place where they select, not a function: as a force-inlined function template the same statements compiled to other
// kernels (the rounds were no longer split into a copy for keep == 1 and one for the rest), and those measured 8 to 12 % slower at
// beam_size 16 on the MI355X.  Included as text the kernels keep their instruction streams.
//
// The including scope provides
//   PMAX, P, keep, lane   the positions the registers are laid out for, those that exist, the keys to keep, the lane
//   u[PMAX * 4]           u[b * 4 + q]: the ordered score (kxb_ordered) of position b < P and the lane's candidate q
//   cand[WAVE], win[PMAX] LDS: the keys within the bound; win[i] = the flat index b * 256 + s of rank i
//   rounds                bool: start in the general way (keep == 1, as a rule)
//   KXB_SELECT_SCORES     1: wins[PMAX] (LDS) takes the score of rank i as an ordered integer; 0: only `top`, the score of rank 0
//                         when the general way ran, is kept
// and its own barrier after the text publishes win[] / wins[].
//
// The 64-bit key is (score bits, b * 256 + s), so the tie rule (equal scores -> smaller flat index) falls out of the key.  One
// hypothesis to keep: a wave-wide minimum.  Several: a round of the general way costs a pass over every key of the lane, so first
// cut the keys down.  T = the keep-th smallest of the 64 lanes' own minima is a score that at least `keep` keys reach, so every key of
// the best `keep` has a score <= T; the keys that do (a few more than `keep`, as a rule) are gathered in LDS and ranked there by
// counting, on the full key.  More than 64 of them (many equal scores) go the general way instead: `keep` rounds, each the wave-wide
// minimum of the keys above the last one taken.  The index half of a key is built from lane and loop counters alone and LDS slots
// from lane counts: no address is ever formed from a score, whatever NaNs make of the order.
      if (!rounds) {
        uint32_t mine = 0xffffffffu;
#pragma unroll
        for (int b = 0; b < PMAX; ++b) {
          if (b < P) {
#pragma unroll
            for (int q = 0; q < kKxbPerLane; ++q) mine = u[b * kKxbPerLane + q] < mine ? u[b * kKxbPerLane + q] : mine;
          }
        }
        uint32_t bound = 0;
        for (int r = 0; r < keep; ++r) {
          bound = kxb_wave_min_u32(mine);
          const unsigned long long at = __builtin_amdgcn_ballot_w64(mine == bound);  // (never empty: some lane holds the minimum)
          if (lane == (int)__builtin_ctzll(at | (1ull << 63))) mine = 0xffffffffu;
        }
        int n = 0;  // wave-uniform
#pragma unroll
        for (int b = 0; b < PMAX; ++b) {
          if (b < P) {
#pragma unroll
            for (int q = 0; q < kKxbPerLane; ++q) {
              const bool in = u[b * kKxbPerLane + q] <= bound;
              const unsigned long long set = __builtin_amdgcn_ballot_w64(in);
              if (set != 0) {  // wave-uniform
                const int at = n + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(set >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)set, 0u));
                if (in && at < WAVE)
                  cand[at] = ((uint64_t)u[b * kKxbPerLane + q] << 32) | (uint32_t)(b * kKxbEntries + kKxbPerLane * lane + q);
                n += (int)__builtin_popcountll(set);
              }
            }
          }
        }
        if (n > WAVE || n < keep) {  // (n < keep cannot happen: `keep` lanes hold a key within the bound)
          rounds = true;
        } else {
          __syncthreads();
          const uint64_t key = lane < n ? cand[lane] : ~0ull;
          int rank = 0;
          for (int i = 0; i < n; ++i) rank += cand[i] < key ? 1 : 0;  // keys are distinct (their index halves are): so are the ranks
          if (lane < n && rank < keep) {
            win[rank] = (uint32_t)key;
#if KXB_SELECT_SCORES
            wins[rank] = (uint32_t)(key >> 32);
#endif
          }
        }
      }
      // the general way: `keep` rounds, each the wave-wide minimum of the keys above the last one taken
      if (rounds) {
        uint64_t taken = 0;
        for (int r = 0; r < keep; ++r) {
          uint64_t best = ~0ull;
#pragma unroll
          for (int b = 0; b < PMAX; ++b) {
            if (b < P) {
#pragma unroll
              for (int q = 0; q < kKxbPerLane; ++q) {
                const uint64_t key = ((uint64_t)u[b * kKxbPerLane + q] << 32) | (uint32_t)(b * kKxbEntries + kKxbPerLane * lane + q);
                const bool ok = (r == 0 || key > taken) && key < best;
                best = ok ? key : best;
              }
            }
          }
          best = kxb_wave_min(best);
          taken = best;
#if KXB_SELECT_SCORES
          if (lane == 0) {
            win[r] = (uint32_t)best;
            wins[r] = (uint32_t)(best >> 32);
          }
#else
          if (r == 0) top = (uint32_t)(best >> 32);
          if (lane == 0) win[r] = (uint32_t)best;
#endif
        }
      }
