// Run successors of the dense backward kernel's run skipping ("Run skipping").  Host only, no HIP: the
// builder is also compiled into a stand-alone program by tests/test_bwd_skip_runs_cpu.py.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace phmm {

// A run is npt consecutive node ids, rho = node / npt: what one row of bwd_step walks.  desc_off / desc is the CSR
// of the nodes each node reaches within the hops of the Del closure (the nodes of the hop entries bh of model.cpp,
// duplicates allowed: the merged closure entries bc name a subset of them).  rs_off / rs becomes the CSR of, per
// run, the sorted OTHER runs that hold such a node of any of its nodes: a backward column can be non-zero in a run
// only where the column before was non-zero in the run itself or in one of these.
inline void build_run_successors(uint32_t N, uint32_t npt, const std::vector<uint32_t> &desc_off,
                                 const std::vector<uint32_t> &desc, std::vector<uint32_t> &rs_off,
                                 std::vector<uint32_t> &rs) {
    const uint32_t nrun = (uint32_t)(((uint64_t)N + npt - 1) / npt);
    rs_off.assign((size_t)nrun + 1, 0);
    rs.clear();
    std::vector<uint32_t> tmp;
    for (uint32_t rho = 0; rho < nrun; rho++) {
        tmp.clear();
        const uint64_t v0 = (uint64_t)rho * npt, v1 = std::min<uint64_t>(v0 + npt, N);
        for (uint32_t q = desc_off[v0]; q < desc_off[v1]; q++) {
            const uint32_t t = desc[q] / npt;
            if (t != rho) tmp.push_back(t);
        }
        std::sort(tmp.begin(), tmp.end());
        tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
        rs.insert(rs.end(), tmp.begin(), tmp.end());
        rs_off[(size_t)rho + 1] = (uint32_t)rs.size();
    }
}

}  // namespace phmm
