"""mkvar.sh patch: k_bp_dfs32<128> at FIVE waves per SIMD -- the LDS stack at 8 and the candidate staging at 4 entries per
thread (16 KiB per workgroup: ten workgroups per CU), __launch_bounds__(128, 5) (96 VGPRs), the grid at ten resident
workgroups per CU.  The other instantiations keep their shape.  With the seed's pose in scalar registers the kernel needs 86
VGPRs, so the bound costs no spill (round 3's attempt at 104 VGPRs spilled 14).  A/B against the product build:
DESIGN section 6, "Radius chains and a scalar pose"."""
p = 'pfc_bp.h'; s = open(p).read()
a = '__global__ void __launch_bounds__(BLK, 4) k_bp_dfs32(Dfs32Args g) {\n    constexpr int kWaves = BLK / 64, kStack = BLK * 10, kOut = BLK * 5;'
assert s.count(a) == 1
s = s.replace(a, '__global__ void __launch_bounds__(BLK, BLK == 128 ? 5 : 4) k_bp_dfs32(Dfs32Args g) {\n'
                 '    constexpr int kWaves = BLK / 64, kStack = BLK * (BLK == 128 ? 8 : 10), kOut = BLK * (BLK == 128 ? 4 : 5);')
open(p, 'w').write(s)
p = 'pfc_hip.hip'; s = open(p).read()
a = '''            if (blk == 128 && f.reserve <= 128 * 10 - 512)
                hipLaunchKernelGGL((k_bp_dfs32<128>), dim3(grid_for(bound, 1, 256 * 8)), dim3(128), 0, st, f);'''
assert s.count(a) == 1
s = s.replace(a, '''            if (blk == 128 && f.reserve <= 128 * 8 - 512)
                hipLaunchKernelGGL((k_bp_dfs32<128>), dim3(grid_for(bound, 1, 256 * 10)), dim3(128), 0, st, f);''')
open(p, 'w').write(s)
