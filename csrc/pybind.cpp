// Python boundary of the MI355X-native sparse tensor engine.
// CPU core functions exposed over torch tensors, and the HIP launchers of
// csrc/hip/*.hip (compiled by hipcc for gfx950 and linked in). The launchers
// are declared once, in csrc/hip/launchers.hpp, which both sides include;
// they take raw device pointers + the current stream, so this translation
// unit needs no HIP headers. Every gpu_* binding validates each tensor it
// takes (check_dev: dtype, device, contiguity) before anything is launched,
// picks the launcher instantiation with by_dtype / by_store, and turns the
// launcher's return value into an exception with check_rc.
#include <torch/extension.h>
#include <array>
#include <string>
#include <vector>

#include "core/types.hpp"
#include "core/sptensor.hpp"
#include "core/csf.hpp"
#include "core/mttkrp_cpu.hpp"
#include "core/matrix.hpp"
#include "core/cpd.hpp"
#include "core/io.hpp"
#include "core/partition.hpp"
#include "hip/launchers.hpp"

namespace sp = splatt;
namespace gpu = splatt::hip;
using torch::Tensor;

// ---------------------------------------------------------------- helpers

// Element types travel as Tag<T> values into generic lambdas.
template <typename T> struct Tag { using type = T; };
#define TAG_TYPE(tag) typename decltype(tag)::type

template <typename T>
static constexpr torch::ScalarType dtype_of() {
  if constexpr (std::is_same<T, gpu::bf16>::value) return torch::kBFloat16;
  else return c10::CppTypeToScalarType<T>::value;
}

// f(Tag<float>) for f32, f(Tag<double>) otherwise
template <typename F>
static auto by_dtype(torch::ScalarType ty, F && f) {
  return ty == torch::kFloat32 ? f(Tag<float>{}) : f(Tag<double>{});
}
template <typename F>
static auto by_dtype(const Tensor & vals, F && f) {
  return by_dtype(vals.scalar_type(), f);
}

// f(Tag<V>, Tag<S>): V from the values, S the factor storage type — V, or
// f32 / bf16 under f64 values (reduced-precision factor STORAGE with f64
// accumulation)
template <typename F>
static auto by_store(const Tensor & vals, const Tensor & mats0, F && f) {
  if (vals.scalar_type() == torch::kFloat64) {
    if (mats0.scalar_type() == torch::kFloat32)
      return f(Tag<double>{}, Tag<float>{});
    if (mats0.scalar_type() == torch::kBFloat16)
      return f(Tag<double>{}, Tag<gpu::bf16>{});
  }
  return by_dtype(vals, [&](auto v) { return f(v, v); });
}

static sp::Options opts_from_dict(const py::dict & d) {
  sp::Options o;
  if (d.contains("tolerance")) o.tolerance = d["tolerance"].cast<double>();
  if (d.contains("max_iters")) o.max_iters = d["max_iters"].cast<uint64_t>();
  if (d.contains("seed")) o.seed = d["seed"].cast<uint64_t>();
  if (d.contains("nthreads")) o.nthreads = d["nthreads"].cast<int>();
  if (d.contains("regularize"))
    o.regularize = d["regularize"].cast<double>();
  if (d.contains("csf_alloc")) {
    const std::string a = d["csf_alloc"].cast<std::string>();
    o.csf_alloc = a == "one" ? sp::CsfAlloc::ONEMODE
                : a == "all" ? sp::CsfAlloc::ALLMODE
                             : sp::CsfAlloc::TWOMODE;
  }
  return o;
}

template <typename V>
static sp::SpTensor<V> coo_from_torch(const Tensor & inds, const Tensor & vals,
                                      const std::vector<int64_t> & dims) {
  TORCH_CHECK(inds.dim() == 2, "inds must be [nmodes, nnz]");
  TORCH_CHECK(inds.scalar_type() == torch::kInt64, "inds must be int64");
  auto ic = inds.contiguous();
  auto vc = vals.contiguous();
  const int nm = (int)ic.size(0);
  const sp::idx_t nnz = (sp::idx_t)ic.size(1);
  sp::idx_t d[sp::MAX_NMODES];
  for (int m = 0; m < nm; ++m) d[m] = (sp::idx_t)dims[m];
  sp::SpTensor<V> tt(nm, nnz, d);
  const int64_t * ip = ic.data_ptr<int64_t>();
  const V * vp = vc.data_ptr<V>();
  for (int m = 0; m < nm; ++m)
    for (sp::idx_t i = 0; i < nnz; ++i) tt.ind[m][i] = (sp::idx_t)ip[m * nnz + i];
  std::copy(vp, vp + nnz, tt.vals.begin());
  return tt;
}

template <typename V>
static std::tuple<Tensor, Tensor, std::vector<int64_t>>
coo_to_torch(const sp::SpTensor<V> & tt) {
  Tensor inds = torch::empty({tt.nmodes, (int64_t)tt.nnz}, torch::kInt64);
  Tensor vals = torch::empty({(int64_t)tt.nnz}, dtype_of<V>());
  int64_t * ip = inds.data_ptr<int64_t>();
  V * vp = vals.data_ptr<V>();
  for (int m = 0; m < tt.nmodes; ++m)
    for (sp::idx_t i = 0; i < tt.nnz; ++i) ip[m * tt.nnz + i] = (int64_t)tt.ind[m][i];
  std::copy(tt.vals.begin(), tt.vals.end(), vp);
  std::vector<int64_t> dims(tt.nmodes);
  for (int m = 0; m < tt.nmodes; ++m) dims[m] = (int64_t)tt.dims[m];
  return {inds, vals, dims};
}

// csf as a python dict of torch tensors
template <typename V>
static py::dict csf_to_py(const sp::Csf<V> & c) {
  py::dict d;
  py::list fptr, fids;
  for (int l = 0; l < c.nmodes; ++l) {
    if (l < c.nmodes - 1) {
      Tensor t = torch::empty({(int64_t)c.fptr[l].size()}, torch::kInt64);
      std::copy(c.fptr[l].begin(), c.fptr[l].end(), t.data_ptr<int64_t>());
      fptr.append(t);
    } else {
      fptr.append(py::none());
    }
    if (c.fids[l].empty()) {
      fids.append(py::none());
    } else {
      Tensor t = torch::empty({(int64_t)c.fids[l].size()}, torch::kInt32);
      const sp::fid_t * s = c.fids[l].data();
      int32_t * p = t.data_ptr<int32_t>();
      for (size_t i = 0; i < c.fids[l].size(); ++i) p[i] = (int32_t)s[i];
      fids.append(t);
    }
  }
  Tensor vals = torch::empty({(int64_t)c.vals.size()}, dtype_of<V>());
  std::copy(c.vals.begin(), c.vals.end(), vals.data_ptr<V>());
  d["fptr"] = fptr;
  d["fids"] = fids;
  d["vals"] = vals;
  std::vector<int64_t> dims(c.nmodes), perm(c.nmodes), nfibs(c.nmodes);
  for (int l = 0; l < c.nmodes; ++l) {
    dims[l] = (int64_t)c.dims[l];
    perm[l] = c.dim_perm[l];
    nfibs[l] = (int64_t)c.nfibs[l];
  }
  d["dims"] = dims;
  d["dim_perm"] = perm;
  d["nfibs"] = nfibs;
  return d;
}

template <typename V>
static sp::Csf<V> csf_from_py(const py::dict & d) {
  sp::Csf<V> c;
  auto dims = d["dims"].cast<std::vector<int64_t>>();
  auto perm = d["dim_perm"].cast<std::vector<int64_t>>();
  c.nmodes = (int)dims.size();
  for (int l = 0; l < c.nmodes; ++l) {
    c.dims[l] = (sp::idx_t)dims[l];
    c.dim_perm[l] = (int)perm[l];
    c.dim_iperm[perm[l]] = l;
  }
  py::list fptr = d["fptr"], fids = d["fids"];
  for (int l = 0; l < c.nmodes; ++l) {
    if (!fptr[l].is_none()) {
      Tensor t = fptr[l].cast<Tensor>().contiguous();
      c.fptr[l].assign(t.data_ptr<int64_t>(), t.data_ptr<int64_t>() + t.numel());
    }
    if (!fids[l].is_none()) {
      Tensor t = fids[l].cast<Tensor>().contiguous();
      const int32_t * p = t.data_ptr<int32_t>();
      c.fids[l].resize(t.numel());
      for (int64_t i = 0; i < t.numel(); ++i) c.fids[l][i] = (sp::fid_t)p[i];
    }
  }
  Tensor vals = d["vals"].cast<Tensor>().contiguous();
  c.vals.assign(vals.data_ptr<V>(), vals.data_ptr<V>() + vals.numel());
  c.nnz = (sp::idx_t)c.vals.size();
  for (int l = 0; l < c.nmodes; ++l)
    c.nfibs[l] = l < c.nmodes - 1 ? (c.fptr[l].empty() ? 0 : c.fptr[l].size() - 1)
                                  : c.nnz;
  return c;
}

// contiguous copies of the factors + their row pointers (CPU kernels)
template <typename V>
struct HostMats {
  std::vector<Tensor> keep;
  std::vector<const V *> ptr;
  explicit HostMats(const std::vector<Tensor> & mats) {
    for (auto & m : mats) {
      keep.push_back(m.contiguous());
      ptr.push_back(keep.back().data_ptr<V>());
    }
  }
};

// ---------------------------------------------------------------- io

static py::object py_tensor_load(const std::string & path, const std::string & dtype) {
  return by_dtype(dtype == "f32" ? torch::kFloat32 : torch::kFloat64,
                  [&](auto tag) -> py::object {
    auto tt = sp::tensor_load<TAG_TYPE(tag)>(path);
    auto [i, v, d] = coo_to_torch(tt);
    return py::make_tuple(i, v, d);
  });
}

static void py_tns_write(const std::string & path, Tensor inds, Tensor vals,
                         std::vector<int64_t> dims) {
  by_dtype(vals, [&](auto tag) {
    sp::tns_write(coo_from_torch<TAG_TYPE(tag)>(inds, vals, dims), path);
  });
}

static void py_bin_write(const std::string & path, Tensor inds, Tensor vals,
                         std::vector<int64_t> dims, int idx_bytes, int val_bytes) {
  by_dtype(vals, [&](auto tag) {
    sp::bin_write(coo_from_torch<TAG_TYPE(tag)>(inds, vals, dims), path,
                  idx_bytes, val_bytes);
  });
}

// ------------------------------------------------------------- coo utils

static py::tuple py_coo_fix(Tensor inds, Tensor vals, std::vector<int64_t> dims,
                            bool dedup, bool compress) {
  return by_dtype(vals, [&](auto tag) {
    auto tt = coo_from_torch<TAG_TYPE(tag)>(inds, vals, dims);
    int64_t ndups = 0, nempty = 0;
    if (dedup) {
      std::vector<int> perm(tt.nmodes);
      for (int m = 0; m < tt.nmodes; ++m) perm[m] = m;
      sp::coo_sort(tt, perm.data());
      ndups = (int64_t)sp::coo_remove_dups(tt);
    }
    py::list indmaps;
    if (compress) {
      nempty = (int64_t)sp::coo_remove_empty(tt);
      for (int m = 0; m < tt.nmodes; ++m) {
        if (tt.indmap[m].empty()) {
          indmaps.append(py::none());
        } else {
          Tensor t = torch::empty({(int64_t)tt.indmap[m].size()}, torch::kInt64);
          std::copy(tt.indmap[m].begin(), tt.indmap[m].end(), t.data_ptr<int64_t>());
          indmaps.append(t);
        }
      }
    }
    auto [i, v, d] = coo_to_torch(tt);
    return py::make_tuple(i, v, d, ndups, nempty, indmaps);
  });
}

// ------------------------------------------------------------- csf build

static py::object py_csf_build(Tensor inds, Tensor vals,
                               std::vector<int64_t> dims,
                               std::vector<int64_t> perm) {
  return by_dtype(vals, [&](auto tag) -> py::object {
    auto tt = coo_from_torch<TAG_TYPE(tag)>(inds, vals, dims);
    int p[sp::MAX_NMODES];
    for (size_t i = 0; i < perm.size(); ++i) p[i] = (int)perm[i];
    return csf_to_py(sp::csf_build(tt, p));
  });
}

// ---------------------------------------------------------------- mttkrp

static Tensor py_mttkrp_stream(Tensor inds, Tensor vals, std::vector<int64_t> dims,
                               std::vector<Tensor> mats, int mode) {
  return by_dtype(vals, [&](auto tag) {
    using V = TAG_TYPE(tag);
    auto tt = coo_from_torch<V>(inds, vals, dims);
    const int F = (int)mats[0].size(1);
    HostMats<V> hm(mats);
    Tensor out = torch::empty({dims[mode], F}, mats[0].options());
    sp::mttkrp_stream(tt, hm.ptr.data(), out.data_ptr<V>(), mode, F);
    return out;
  });
}

static Tensor py_mttkrp_csf(py::dict csf, std::vector<Tensor> mats, int mode,
                            int nthreads) {
  return by_dtype(mats[0], [&](auto tag) {
    using V = TAG_TYPE(tag);
    auto c = csf_from_py<V>(csf);
    const int F = (int)mats[0].size(1);
    HostMats<V> hm(mats);
    Tensor out = torch::empty({(int64_t)c.dims[mode], F}, mats[0].options());
    sp::mttkrp_csf_cpu(c, hm.ptr.data(), out.data_ptr<V>(), mode, F, nthreads);
    return out;
  });
}

// ------------------------------------------------------------------- cpd

static py::dict py_cpd_als(Tensor inds, Tensor vals, std::vector<int64_t> dims,
                           int rank, py::dict opts) {
  return by_dtype(vals, [&](auto tag) {
    using V = TAG_TYPE(tag);
    auto o = opts_from_dict(opts);
    auto tt = coo_from_torch<V>(inds, vals, dims);
    auto set = sp::csf_alloc(tt, o);
    auto k = sp::cpd_als(set, rank, o);
    py::dict r;
    py::list factors;
    for (int m = 0; m < k.nmodes; ++m) {
      Tensor t = torch::empty({(int64_t)k.dims[m], rank}, dtype_of<V>());
      std::copy(k.factors[m].begin(), k.factors[m].end(), t.data_ptr<V>());
      factors.append(t);
    }
    Tensor lam = torch::empty({rank}, dtype_of<V>());
    std::copy(k.lambda.begin(), k.lambda.end(), lam.data_ptr<V>());
    r["factors"] = factors;
    r["lambda"] = lam;
    r["fit"] = k.fit;
    r["niters"] = k.niters;
    return r;
  });
}

// --------------------------------------------------------------- dense ops

static Tensor py_seeded_init(int64_t nrows, int rank, int64_t row0,
                             uint64_t seed, int mode, const std::string & dtype) {
  return by_dtype(dtype == "f32" ? torch::kFloat32 : torch::kFloat64,
                  [&](auto tag) {
    using V = TAG_TYPE(tag);
    Tensor t = torch::empty({nrows, rank}, dtype_of<V>());
    sp::seeded_factor_init(t.data_ptr<V>(), (sp::idx_t)nrows, rank,
                           (sp::idx_t)row0, seed, mode);
    return t;
  });
}

static std::vector<int64_t> py_order_modes(std::vector<int64_t> dims,
                                           const std::string & policy, int mode) {
  const int nm = (int)dims.size();
  sp::idx_t d[sp::MAX_NMODES];
  for (int m = 0; m < nm; ++m) d[m] = (sp::idx_t)dims[m];
  int p[sp::MAX_NMODES];
  if (policy == "smallfirst") sp::order_smallfirst(d, nm, p);
  else if (policy == "root") sp::order_root(d, nm, mode, p);
  else sp::order_leaf(d, nm, mode, p);
  return std::vector<int64_t>(p, p + nm);
}

// ------------------------------------------------- HIP launcher plumbing
// Python passes device tensors + the current stream's handle.

static void check_dev(const Tensor & t, torch::ScalarType ty,
                      const char * name) {
  TORCH_CHECK(t.scalar_type() == ty, name, " has dtype ", t.scalar_type(),
              ", expected ", ty);
  TORCH_CHECK(t.is_cuda(), name, " must be a device tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

// device pointer of a checked tensor; the one place a bf16 tensor becomes
// the launchers' bf16
template <typename T>
static T * dev_ptr(const Tensor & t, const char * name) {
  check_dev(t, dtype_of<T>(), name);
  if constexpr (std::is_same<T, gpu::bf16>::value)
    return reinterpret_cast<gpu::bf16 *>(t.data_ptr<at::BFloat16>());
  else
    return t.data_ptr<T>();
}

// Host table of the device pointers of tensors[0, n), each checked; always
// 8 entries, the unused ones null, as the launchers expect.
template <typename T>
static std::array<const T *, 8> ptr_table(const std::vector<Tensor> & tensors,
                                          size_t n, const char * name) {
  TORCH_CHECK(n <= 8 && tensors.size() == n, "expected ", n, " ", name,
              " tensors, got ", tensors.size());
  std::array<const T *, 8> tab{};
  for (size_t t = 0; t < n; ++t) tab[t] = dev_ptr<T>(tensors[t], name);
  return tab;
}

// the per-nonzero int32 index streams of a launch: nnz entries each
static std::array<const int32_t *, 8> stream_table(
    const std::vector<Tensor> & idx, size_t n, int64_t nnz) {
  auto tab = ptr_table<int32_t>(idx, n, "idx");
  for (auto & i : idx)
    TORCH_CHECK(i.numel() == nnz, "index stream length != nnz");
  return tab;
}

// the factor matrices of a launch: [rows, rank] each
template <typename S>
static std::array<const S *, 8> factor_table(const std::vector<Tensor> & mats,
                                             size_t n, int64_t rank) {
  auto tab = ptr_table<S>(mats, n, "factor");
  for (auto & m : mats)
    TORCH_CHECK(m.dim() == 2 && m.size(1) == rank, "factor rank mismatch");
  return tab;
}

// rank of a launch = columns of its first factor
static int rank_of(const std::vector<Tensor> & mats) {
  TORCH_CHECK(!mats.empty() && mats[0].dim() == 2, "factors must be 2-D");
  return (int)mats[0].size(1);
}

// `out` of an MTTKRP: [rows, rank]
template <typename V>
static V * out_ptr(const Tensor & out, int rank) {
  V * p = dev_ptr<V>(out, "out");
  TORCH_CHECK(out.dim() == 2 && out.size(1) == rank,
              "out must be [rows, rank]");
  return p;
}

// A launcher's return value (launchers.hpp) as an exception: positive = the
// launch's hipError_t, negative = declined, with the binding's message.
static void check_rc(int rc, const char * what, const std::string & declined) {
  TORCH_CHECK(rc <= 0, what, " kernel launch failed: ", gpu::error_string(rc));
  TORCH_CHECK(rc == 0, declined);
}
// for launchers that never decline
static void check_rc(int rc, const char * what) {
  check_rc(rc, what, std::string(what) + " launcher declined");
}

// block descriptors of the LDS-staged kernels (mttkrp.py _stage_blocks)
struct StageBlocks {
  const int64_t * start, * end;
  const int32_t * row0;
  int64_t n;
  StageBlocks(const Tensor & blk_start, const Tensor & blk_end,
              const Tensor & blk_row0)
      : start(dev_ptr<int64_t>(blk_start, "blk_start")),
        end(dev_ptr<int64_t>(blk_end, "blk_end")),
        row0(dev_ptr<int32_t>(blk_row0, "blk_row0")), n(blk_start.numel()) {
    TORCH_CHECK(blk_end.numel() == n && blk_row0.numel() == n,
                "block descriptor lengths differ");
  }
};

// the packed stream of flat6 / det6: one int4 word per nonzero
static const int32_t * pack_ptr(const Tensor & pack, int64_t nnz) {
  TORCH_CHECK(pack.dim() == 2 && pack.size(1) == 4 && pack.is_contiguous()
              && pack.scalar_type() == torch::kInt32,
              "pack must be contiguous [nnz,4] int32");
  const int32_t * p = dev_ptr<int32_t>(pack, "pack");
  TORCH_CHECK(pack.size(0) == nnz, "pack length != nnz");
  return p;
}

static const int64_t * rowptr_ptr(const Tensor & rowptr, const Tensor & out) {
  const int64_t * p = dev_ptr<int64_t>(rowptr, "rowptr");
  TORCH_CHECK(rowptr.numel() >= 2 && out.dim() == 2
              && rowptr.numel() <= out.size(0) + 1,
              "rowptr must be contiguous int64 with at most rows + 1 entries");
  return p;
}

// ------------------------------------------------------------ MTTKRP (HIP)

// 3-mode CSF walk; which: 0 root, 1 internal, 2 leaf output
static void py_gpu_mttkrp3(int which, Tensor fptr0, py::object fids0, Tensor fptr1,
                           Tensor fids1, Tensor fids2, Tensor vals,
                           Tensor Ma, Tensor Mb, Tensor out, int64_t stream) {
  TORCH_CHECK(which >= 0 && which <= 2, "which: 0 root, 1 internal, 2 leaf");
  by_dtype(vals, [&](auto tag) {
    using V = TAG_TYPE(tag);
    const int64_t * fp0 = dev_ptr<int64_t>(fptr0, "fptr0");
    const int32_t * f0 = fids0.is_none() ? nullptr
                         : dev_ptr<int32_t>(fids0.cast<Tensor>(), "fids0");
    const int64_t * fp1 = dev_ptr<int64_t>(fptr1, "fptr1");
    const int32_t * fi1 = dev_ptr<int32_t>(fids1, "fids1");
    const int32_t * fi2 = dev_ptr<int32_t>(fids2, "fids2");
    const V * vp = dev_ptr<V>(vals, "vals");
    const V * a = dev_ptr<V>(Ma, "Ma");
    const V * b = dev_ptr<V>(Mb, "Mb");
    const int64_t nslices = fptr0.numel() - 1;
    const int64_t nfibs = fptr1.numel() - 1;
    const int64_t nnz = vals.numel();
    TORCH_CHECK(fids1.numel() == nfibs && fids2.numel() == nnz,
                "fids1/fids2 lengths != fibers/nnz");
    TORCH_CHECK(Ma.dim() == 2 && Mb.dim() == 2 && Mb.size(1) == Ma.size(1),
                "factor rank mismatch");
    const int rank = (int)Ma.size(1);
    check_rc(gpu::mttkrp_csf3<V>(which, fp0, f0, fp1, fi1, fi2, vp, nslices,
                                 nfibs, nnz, a, b, out_ptr<V>(out, rank),
                                 rank, (void *)stream), "mttkrp3");
  });
}

// The key-stream / row-pointer forms of the flat kernel share this: exactly
// one of key / rowptr is given. Returns the launcher's return value.
template <typename V, typename S, typename VS>
static int flat_launch(const c10::optional<Tensor> & rowptr, int64_t p0,
                       const c10::optional<Tensor> & key,
                       const std::vector<Tensor> & idx,
                       const std::vector<Tensor> & mats, const Tensor & vals,
                       const Tensor & out, int64_t stream) {
  const size_t nother = idx.size();
  TORCH_CHECK(nother >= 2 && nother <= 7, "flat kernel supports 3..8 modes");
  TORCH_CHECK(rowptr.has_value() != key.has_value(),
              "pass row pointers or a key stream, not both");
  const VS * vp = dev_ptr<VS>(vals, "vals");
  const int64_t nnz = vals.numel();
  const int rank = rank_of(mats);
  V * op = out_ptr<V>(out, rank);
  auto ip = stream_table(idx, nother, nnz);
  auto mp = factor_table<S>(mats, nother, rank);
  const int32_t * kp = nullptr;
  const int64_t * rp = nullptr;
  if (key.has_value()) {
    kp = dev_ptr<int32_t>(*key, "key");
    TORCH_CHECK(key->numel() == nnz, "key must be int32 of nnz entries");
  } else {
    rp = rowptr_ptr(*rowptr, out);
  }
  return gpu::mttkrp_flat<V, S, VS>(kp, rp, rp ? rowptr->numel() - 1 : 0, p0,
                                    ip.data(), mp.data(), vp, nnz, op, rank,
                                    (int)nother, (void *)stream);
}

// key + per-other-level (idx, mat) pairs; nnz products folded by key runs
static void py_gpu_mttkrp_flat(Tensor key, std::vector<Tensor> idx,
                               std::vector<Tensor> mats, Tensor vals,
                               Tensor out, int64_t stream) {
  TORCH_CHECK(!mats.empty(), "flat kernel supports 3..8 modes");
  by_store(vals, mats[0], [&](auto v, auto s) {
    using V = TAG_TYPE(v);
    using S = TAG_TYPE(s);
    const int rc = flat_launch<V, S, V>(c10::nullopt, 0, key, idx, mats, vals,
                                        out, stream);
    check_rc(rc, "flat MTTKRP",
             std::string(std::is_same<S, float>::value ? "f32" : "bf16")
             + " factor store needs rank in {4,8,16,32,64}");
  });
}

// Row-pointer form of the flat kernel: `rowptr` (int64, rows + 1 global
// stream positions) replaces the key stream; idx/vals are the launch's
// slices starting at global stream position p0. Returns false when the
// launch does not qualify (the caller then takes gpu_mttkrp_flat).
static bool py_gpu_mttkrp_flat_rp(Tensor rowptr, int64_t p0,
                                  std::vector<Tensor> idx,
                                  std::vector<Tensor> mats, Tensor vals,
                                  Tensor out, int64_t stream) {
  TORCH_CHECK(!mats.empty(), "flat kernel supports 3..8 modes");
  return by_store(vals, mats[0], [&](auto v, auto s) {
    using V = TAG_TYPE(v);
    const int rc = flat_launch<V, TAG_TYPE(s), V>(rowptr, p0, c10::nullopt,
                                                  idx, mats, vals, out,
                                                  stream);
    if (rc > 0) check_rc(rc, "flat MTTKRP");
    return rc == 0;
  });
}

// f32 value stream of an f64 tensor (values all f32-exact, narrowed once by
// the caller): the v7 kernel with row pointers (`rowptr` given) or the key
// stream. Factors and output stay f64. Returns false when the launch does
// not qualify for v7 — the caller then runs the 8-byte stream.
static bool py_gpu_mttkrp_flat_v32(c10::optional<Tensor> rowptr, int64_t p0,
                                   c10::optional<Tensor> key,
                                   std::vector<Tensor> idx,
                                   std::vector<Tensor> mats, Tensor vals32,
                                   Tensor out, int64_t stream) {
  const int rc = flat_launch<double, double, float>(rowptr, p0, key, idx, mats,
                                                    vals32, out, stream);
  if (rc > 0) check_rc(rc, "flat MTTKRP");
  return rc == 0;
}

// Strip/window flat MTTKRP (csrc/hip/mttkrp_strip.hip): the strip
// descriptors of splatt_amd/csf.py (device arrays), f64 or f32 value stream,
// f64 factors and output. Returns false when the launcher declines
// (misaligned streams, tile above the LDS limit) — the caller then takes the
// key-stream kernel. `pace` (96 words of uint32 or int32, or None: no
// waits) and `pace_us` are the pace buffer and wait budget of launchers.hpp;
// `slots` (256 words, or None), `ahead` and `trace` (4 words per workgroup,
// or None) its slot ring, run-ahead and per-workgroup trace.
static bool py_mttkrp_strip_gpu(Tensor key, std::vector<Tensor> idx,
                                std::vector<Tensor> mats, Tensor vals,
                                Tensor s_row0, Tensor s_nrows, Tensor s_flags,
                                Tensor s_bounds, int64_t tile_rows,
                                int64_t wgs, Tensor out, int64_t stream,
                                c10::optional<Tensor> pace, int64_t pace_us,
                                c10::optional<Tensor> slots, int64_t ahead,
                                c10::optional<Tensor> trace) {
  const size_t nother = idx.size();
  TORCH_CHECK(nother >= 2 && nother <= 3, "strip kernel supports 3..4 modes");
  TORCH_CHECK(tile_rows >= 1 && tile_rows <= (1 << 20) && wgs >= 1
              && wgs <= (1 << 20), "tile_rows / wgs out of range");
  const int64_t nnz = vals.numel();
  const int rank = rank_of(mats);
  double * op = out_ptr<double>(out, rank);
  auto ip = stream_table(idx, nother, nnz);
  auto mp = factor_table<double>(mats, nother, rank);
  const int32_t * kp = dev_ptr<int32_t>(key, "key");
  TORCH_CHECK(key.numel() == nnz, "key must be int32 of nnz entries");
  const int32_t * r0 = dev_ptr<int32_t>(s_row0, "strip row0");
  const int32_t * nr = dev_ptr<int32_t>(s_nrows, "strip nrows");
  const int32_t * fl = dev_ptr<int32_t>(s_flags, "strip flags");
  const int64_t * bp = dev_ptr<int64_t>(s_bounds, "strip bounds");
  const int64_t ns = s_row0.numel();
  TORCH_CHECK(s_nrows.numel() == ns && s_flags.numel() == ns
              && s_bounds.dim() == 2 && s_bounds.size(0) == ns
              && s_bounds.size(1) >= 2 && s_bounds.size(1) <= (1 << 16),
              "strip descriptor lengths differ");
  const int ng = (int)s_bounds.size(1) - 1;
  uint32_t * pp = nullptr;
  if (pace.has_value()) {
    const Tensor & p = *pace;
    TORCH_CHECK(p.is_cuda(), "pace must be a device tensor");
    TORCH_CHECK(p.scalar_type() == torch::kInt32
                || p.scalar_type() == at::ScalarType::UInt32,
                "pace has dtype ", p.scalar_type(), ", expected Int or UInt32");
    TORCH_CHECK(p.is_contiguous() && p.numel() >= 96,
                "pace must be contiguous and hold at least 96 words");
    pp = static_cast<uint32_t *>(p.data_ptr());
  }
  TORCH_CHECK(pace_us >= 0 && pace_us <= 60 * 1000 * 1000,
              "pace_us out of range");
  // words of a pace-side buffer: device, 32-bit integers, contiguous
  auto words = [](const Tensor & p, const char * what, int64_t need) {
    TORCH_CHECK(p.is_cuda(), what, " must be a device tensor");
    TORCH_CHECK(p.scalar_type() == torch::kInt32
                || p.scalar_type() == at::ScalarType::UInt32,
                what, " has dtype ", p.scalar_type(),
                ", expected Int or UInt32");
    TORCH_CHECK(p.is_contiguous() && p.numel() >= need, what,
                " must be contiguous and hold at least ", need, " words");
    return static_cast<uint32_t *>(p.data_ptr());
  };
  TORCH_CHECK(ahead >= 0 && ahead <= 7, "ahead out of range 0..7");
  uint32_t * sp_ = nullptr, * tp = nullptr;
  if (slots.has_value()) {
    TORCH_CHECK(pp != nullptr, "slots need a pace tensor");
    sp_ = words(*slots, "slots", 256);
  }
  TORCH_CHECK(ahead == 0 || sp_ != nullptr,
              "ahead > 0 needs pace and slots tensors");
  if (trace.has_value()) {
    TORCH_CHECK(pp != nullptr, "trace needs a pace tensor");
    tp = words(*trace, "trace", 4 * std::min<int64_t>(wgs, ns));
  }
  const int rc = vals.scalar_type() == torch::kFloat32
      ? gpu::mttkrp_strip<float>(kp, ip.data(), mp.data(),
                                 dev_ptr<float>(vals, "vals"), r0, nr, fl, bp,
                                 ng, ns, (int)tile_rows, (int)wgs, nnz, op,
                                 rank, (int)nother, (void *)stream, pp,
                                 (int)pace_us, sp_, (int)ahead, tp)
      : gpu::mttkrp_strip<double>(kp, ip.data(), mp.data(),
                                  dev_ptr<double>(vals, "vals"), r0, nr, fl,
                                  bp, ng, ns, (int)tile_rows, (int)wgs, nnz,
                                  op, rank, (int)nother, (void *)stream, pp,
                                  (int)pace_us, sp_, (int)ahead, tp);
  if (rc > 0) check_rc(rc, "strip MTTKRP");
  return rc == 0;
}

// strips of a root-sorted stream (core/partition.hpp plan_strips): rowptr is
// a host int64 tensor of rows + 1 entries
static py::dict py_plan_strips(Tensor rowptr, int64_t tile_rows,
                               int64_t nnz_cap) {
  TORCH_CHECK(!rowptr.is_cuda() && rowptr.scalar_type() == torch::kInt64
              && rowptr.is_contiguous() && rowptr.numel() >= 1,
              "rowptr must be a contiguous host int64 tensor");
  TORCH_CHECK(tile_rows >= 1 && nnz_cap >= 1, "tile_rows, nnz_cap >= 1");
  const sp::Strips s = sp::plan_strips(rowptr.data_ptr<int64_t>(),
                                       rowptr.numel() - 1, tile_rows, nnz_cap);
  auto t32 = [](const std::vector<int32_t> & v) {
    return torch::tensor(v, torch::kInt32);
  };
  auto t64 = [](const std::vector<int64_t> & v) {
    return torch::tensor(v, torch::kInt64);
  };
  py::dict d;
  d["row0"] = t32(s.row0);
  d["nrows"] = t32(s.nrows);
  d["flags"] = t32(s.flags);
  d["p0"] = t64(s.p0);
  d["p1"] = t64(s.p1);
  return d;
}

// deterministic flat MTTKRP (csrc/hip/mttkrp_det.hip): plain stores for
// walker-interior key runs + ordered fixup of boundary partials in `side`
static void py_gpu_mttkrp_flat_det(Tensor key, std::vector<Tensor> idx,
                                   std::vector<Tensor> mats, Tensor vals,
                                   Tensor out, Tensor side, int64_t stream) {
  const size_t nother = idx.size();
  TORCH_CHECK(nother >= 2 && nother <= 4,
              "deterministic kernel supports 3..5 modes");
  by_dtype(vals, [&](auto tag) {
    using V = TAG_TYPE(tag);
    const V * vp = dev_ptr<V>(vals, "vals");
    const int64_t nnz = vals.numel();
    const int rank = rank_of(mats);
    const int32_t * kp = dev_ptr<int32_t>(key, "key");
    TORCH_CHECK(key.numel() == nnz, "key must be int32 of nnz entries");
    auto ip = stream_table(idx, nother, nnz);
    auto mp = factor_table<V>(mats, nother, rank);
    const int rc = gpu::mttkrp_flat_det<V>(
        kp, ip.data(), mp.data(), vp, nnz, out_ptr<V>(out, rank),
        dev_ptr<V>(side, "side"), side.numel(), rank, (int)nother,
        (void *)stream);
    if (rc == -2)
      check_rc(rc, "deterministic MTTKRP", c10::str(
          "deterministic workspace too small (", side.numel(), " elems < ",
          gpu::flat_det_ws(nnz, rank), ")"));
    check_rc(rc, "deterministic MTTKRP", "deterministic kernel requires rank "
             "in {4,8,16,32,64} and <= 5 modes");
  });
}

// LDS-staged variant: idx[0]/mats[0] is the bucketed level; block
// descriptors carry (nnz range, bucket row0)
static void py_gpu_mttkrp_flat5(Tensor key, std::vector<Tensor> idx,
                                std::vector<Tensor> mats, Tensor vals,
                                Tensor blk_start, Tensor blk_end,
                                Tensor blk_row0, int64_t chunk, int64_t dim0,
                                Tensor out, int64_t stream) {
  const size_t nother = idx.size();
  TORCH_CHECK(nother >= 2 && nother <= 4, "flat5 supports 3..5 modes");
  by_dtype(vals, [&](auto tag) {
    using V = TAG_TYPE(tag);
    const V * vp = dev_ptr<V>(vals, "vals");
    const int64_t nnz = vals.numel();
    const int rank = rank_of(mats);
    const int32_t * kp = dev_ptr<int32_t>(key, "key");
    TORCH_CHECK(key.numel() == nnz, "key must be int32 of nnz entries");
    auto ip = stream_table(idx, nother, nnz);
    auto mp = factor_table<V>(mats, nother, rank);
    const StageBlocks blk(blk_start, blk_end, blk_row0);
    check_rc(gpu::mttkrp_flat5<V>(kp, ip.data(), mp.data(), vp, blk.start,
                                  blk.end, blk.row0, blk.n, (int32_t)chunk,
                                  (int32_t)dim0, out_ptr<V>(out, rank), rank,
                                  (int)nother, (void *)stream), "flat5");
  });
}

// packed-stream LDS variant: one int4 word per nonzero
// (x = output key, y = staged level, z/w = remaining levels)
static void py_gpu_mttkrp_flat6(Tensor pack, std::vector<Tensor> mats,
                                Tensor vals, Tensor blk_start,
                                Tensor blk_end, Tensor blk_row0,
                                int64_t chunk, int64_t dim0, Tensor out,
                                int64_t stream) {
  const size_t nother = mats.size();
  TORCH_CHECK(nother >= 2 && nother <= 3, "flat6 supports 3..4 modes");
  by_store(vals, mats[0], [&](auto v, auto s) {
    using V = TAG_TYPE(v);
    using S = TAG_TYPE(s);
    const V * vp = dev_ptr<V>(vals, "vals");
    const int32_t * pp = pack_ptr(pack, vals.numel());
    const int rank = rank_of(mats);
    auto mp = factor_table<S>(mats, nother, rank);
    const StageBlocks blk(blk_start, blk_end, blk_row0);
    check_rc(gpu::mttkrp_flat6<V, S>(pp, mp.data(), vp, blk.start, blk.end,
                                     blk.row0, blk.n, (int32_t)chunk,
                                     (int32_t)dim0, out_ptr<V>(out, rank),
                                     rank, (int)nother, (void *)stream),
             "flat6");
  });
}

// LDS-staged bitwise-deterministic MTTKRP over the packed stream:
// per-bucket privatized outputs + ordered fixup + ascending-bucket fold
static void py_gpu_mttkrp_det6(Tensor pack, std::vector<Tensor> mats,
                               Tensor vals, Tensor blk_start,
                               Tensor blk_end, Tensor blk_row0,
                               Tensor blk_bucket_p0,
                               int64_t chunk, int64_t dim0,
                               int64_t nbuckets, Tensor outb, Tensor side,
                               Tensor out, int64_t stream) {
  const size_t nother = mats.size();
  TORCH_CHECK(nother >= 2 && nother <= 3, "det6 supports 3..4 modes");
  by_dtype(vals, [&](auto tag) {
    using V = TAG_TYPE(tag);
    const V * vp = dev_ptr<V>(vals, "vals");
    const int32_t * pp = pack_ptr(pack, vals.numel());
    const int rank = rank_of(mats);
    auto mp = factor_table<V>(mats, nother, rank);
    const StageBlocks blk(blk_start, blk_end, blk_row0);
    const int64_t * bp0 = dev_ptr<int64_t>(blk_bucket_p0, "blk_bucket_p0");
    TORCH_CHECK(blk_bucket_p0.numel() == blk.n,
                "block descriptor lengths differ");
    V * op = out_ptr<V>(out, rank);
    const int64_t nrows_out = out.size(0);
    V * ob = dev_ptr<V>(outb, "outb");
    V * sd = dev_ptr<V>(side, "side");
    // what the launcher zeroes and the kernels then write (launchers.hpp)
    TORCH_CHECK(rank >= 1 && nbuckets >= 0
                && outb.numel() >= nbuckets * nrows_out * rank
                && side.numel() >= blk.n * 4 * (64 / rank) * 2 * rank,
                "det6 workspace too small");
    const int rc = gpu::mttkrp_det6<V>(
        pp, mp.data(), vp, blk.start, blk.end, blk.row0, bp0, blk.n,
        (int32_t)chunk, (int32_t)dim0, nrows_out, nbuckets, ob, sd, op, rank,
        (int)nother, (void *)stream);
    check_rc(rc, "det6",
             c10::str("det6 supports spec ranks and 3-4 modes, rc=", rc));
  });
}

// --------------------------------------------------------- dense ops (HIP)

// A [n, F] of a dense kernel; returns F
static int dense_rank(const Tensor & A, const char * name) {
  TORCH_CHECK(A.dim() == 2 && A.size(1) >= 1, name, " must be [n, F]");
  return (int)A.size(1);
}

// G (FxF, pre-zeroed) += A^T A for tall-skinny device A
static void py_gpu_gram(Tensor A, Tensor G, int64_t stream) {
  by_dtype(A, [&](auto tag) {
    using V = TAG_TYPE(tag);
    const V * a = dev_ptr<V>(A, "A");
    const int F = dense_rank(A, "A");
    TORCH_CHECK(F <= 64 && G.numel() == (int64_t)F * F,
                "G must be [F, F] with F <= 64");
    check_rc(gpu::gram<V>(a, A.size(0), F, dev_ptr<V>(G, "G"),
                          (void *)stream), "gram");
  });
}

static void py_gpu_gram_det(Tensor A, Tensor Gpart, Tensor G, int64_t stream) {
  by_dtype(A, [&](auto tag) {
    using V = TAG_TYPE(tag);
    const V * a = dev_ptr<V>(A, "A");
    const int F = dense_rank(A, "A");
    V * gp = dev_ptr<V>(Gpart, "Gpart");
    const int64_t nparts = Gpart.numel() / (F * F);
    TORCH_CHECK(nparts >= 1, "gram_det workspace too small");
    TORCH_CHECK(G.numel() == (int64_t)F * F, "G must be [F, F]");
    check_rc(gpu::gram_det<V>(a, A.size(0), F, gp, nparts,
                              dev_ptr<V>(G, "G"), (void *)stream),
             "gram_det");
  });
}

static void py_gpu_rowsolve(Tensor A, Tensor B, Tensor C, int64_t stream) {
  by_dtype(A, [&](auto tag) {
    using V = TAG_TYPE(tag);
    const V * a = dev_ptr<V>(A, "A");
    const int F = dense_rank(A, "A");
    const V * b = dev_ptr<V>(B, "B");
    V * c = dev_ptr<V>(C, "C");
    TORCH_CHECK(B.numel() == (int64_t)F * F, "B must be [F, F]");
    TORCH_CHECK(C.numel() == A.numel(), "C must have the shape of A");
    check_rc(gpu::rowsolve<V>(a, b, c, A.size(0), F, (void *)stream),
             "rowsolve",
             c10::str("rowsolve supports F in {4,8,16,32,64}, got ", F));
  });
}

static void py_gpu_spd_inverse(Tensor G, Tensor Ginv, int64_t stream) {
  by_dtype(G, [&](auto tag) {
    using V = TAG_TYPE(tag);
    const V * g = dev_ptr<V>(G, "G");
    TORCH_CHECK(G.dim() == 2 && G.size(0) == G.size(1) && G.size(0) <= 64
                && Ginv.numel() == G.numel(),
                "G and Ginv must be [F, F] with F <= 64");
    check_rc(gpu::spd_inverse<V>(g, dev_ptr<V>(Ginv, "Ginv"), (int)G.size(0),
                                 (void *)stream), "spd_inverse");
  });
}

// column helpers of the C-API device driver (csrc/capi/capi_gpu.cpp)
static void py_gpu_colacc(Tensor A, int which, Tensor out, int64_t stream) {
  check_dev(A, torch::kFloat64, "A");
  check_dev(out, torch::kFloat64, "out");
  TORCH_CHECK(A.dim() == 2 && A.size(1) >= 1 && A.size(1) <= 64,
              "A must be [n, F] with 1 <= F <= 64");
  TORCH_CHECK(out.numel() == A.size(1), "out length != F");
  TORCH_CHECK(which == 0 || which == 1,
              "which: 0 = sum of squares, 1 = max |x|");
  check_rc(gpu::colacc(A.data_ptr<double>(), A.size(0), (int)A.size(1), which,
                       out.data_ptr<double>(), (void *)stream), "colacc");
}

static void py_gpu_colscale(Tensor A, Tensor lam, int64_t stream) {
  check_dev(A, torch::kFloat64, "A");
  check_dev(lam, torch::kFloat64, "lam");
  TORCH_CHECK(A.dim() == 2 && A.size(1) >= 1 && A.size(1) <= 64,
              "A must be [n, F] with 1 <= F <= 64");
  TORCH_CHECK(lam.numel() == A.size(1), "lam length != F");
  check_rc(gpu::colscale(A.data_ptr<double>(), A.size(0), (int)A.size(1),
                         lam.data_ptr<double>(), (void *)stream), "colscale");
}

static void py_gpu_coldot(Tensor X, Tensor A, Tensor out, int64_t stream) {
  check_dev(X, torch::kFloat64, "X");
  check_dev(A, torch::kFloat64, "A");
  check_dev(out, torch::kFloat64, "out");
  TORCH_CHECK(A.dim() == 2 && A.size(1) >= 1 && A.size(1) <= 64,
              "A must be [n, F] with 1 <= F <= 64");
  TORCH_CHECK(X.dim() == 2 && X.size(0) == A.size(0)
              && X.size(1) == A.size(1), "X and A shapes differ");
  TORCH_CHECK(out.numel() == A.size(1), "out length != F");
  check_rc(gpu::coldot(X.data_ptr<double>(), A.data_ptr<double>(), A.size(0),
                       (int)A.size(1), out.data_ptr<double>(),
                       (void *)stream), "coldot");
}

// --------------------------- segment batches (completion, TTMc; f64 only)

// One batch of a root-sorted stream cut into segments: segments
// [seg0, seg0+nseg) accumulate, then multi-segment rows [m0, m0+nm) are
// folded from the workspace, where slots slot0..slot0+nslots-1 (slot_elems
// doubles each) live during this batch.
struct SegBatch {
  const int64_t * seg_start;
  const int32_t * seg_len, * seg_row, * seg_slot, * mrow;
  const int64_t * mslot;
  double * ws;
  SegBatch(const Tensor & seg_start_, const Tensor & seg_len_,
           const Tensor & seg_row_, const Tensor & seg_slot_, int64_t seg0,
           int64_t nseg, const Tensor & mrow_, const Tensor & mslot_,
           int64_t m0, int64_t nm, int64_t slot0, int64_t nslots,
           const Tensor & ws_, int64_t slot_elems, const char * ws_msg)
      : seg_start(dev_ptr<int64_t>(seg_start_, "seg_start")),
        seg_len(dev_ptr<int32_t>(seg_len_, "seg_len")),
        seg_row(dev_ptr<int32_t>(seg_row_, "seg_row")),
        seg_slot(dev_ptr<int32_t>(seg_slot_, "seg_slot")),
        mrow(dev_ptr<int32_t>(mrow_, "mrow")),
        mslot(dev_ptr<int64_t>(mslot_, "mslot")),
        ws(dev_ptr<double>(ws_, "ws")) {
    TORCH_CHECK(seg_len_.numel() == seg_start_.numel()
                && seg_row_.numel() == seg_start_.numel()
                && seg_slot_.numel() == seg_start_.numel());
    TORCH_CHECK(seg0 >= 0 && nseg >= 0 && seg0 + nseg <= seg_start_.numel(),
                "segment range out of bounds");
    TORCH_CHECK(m0 >= 0 && nm >= 0 && m0 + nm <= mrow_.numel()
                && mslot_.numel() == mrow_.numel() + 1,
                "multi-segment row range out of bounds");
    TORCH_CHECK(nslots >= 0 && slot0 >= 0
                && ws_.numel() >= nslots * slot_elems, ws_msg);
  }
};

// One batch of the row-wise completion update for a root-sorted stream:
// segments accumulate (and solve single-segment rows), then multi-segment
// rows are folded from `ws` and solved.
static void py_gpu_complete_update(
    std::vector<Tensor> idx, std::vector<Tensor> mats, Tensor vals,
    Tensor seg_start, Tensor seg_len, Tensor seg_row, Tensor seg_slot,
    int64_t seg0, int64_t nseg, Tensor mrow, Tensor mslot, int64_t m0,
    int64_t nm, int64_t slot0, int64_t nslots, double reg, Tensor ws,
    Tensor out, int64_t stream) {
  const size_t nother = idx.size();
  TORCH_CHECK(nother >= 2 && nother <= 7, "completion supports 3..8 modes");
  TORCH_CHECK(reg > 0.0, "reg must be > 0");
  const double * vp = dev_ptr<double>(vals, "vals");
  double * op = dev_ptr<double>(out, "out");
  TORCH_CHECK(out.dim() == 2, "out must be [rows, rank]");
  const int F = (int)out.size(1);
  TORCH_CHECK(F >= 1 && F <= 64, "completion supports rank 1..64, got ", F);
  auto ip = stream_table(idx, nother, vals.numel());
  auto mp = factor_table<double>(mats, nother, F);
  const SegBatch b(seg_start, seg_len, seg_row, seg_slot, seg0, nseg, mrow,
                   mslot, m0, nm, slot0, nslots, ws,
                   gpu::complete_slot_elems(F),
                   "completion workspace too small");
  check_rc(gpu::complete_segments(
               ip.data(), mp.data(), (int)nother, vp, b.seg_start, b.seg_len,
               b.seg_row, b.seg_slot, seg0, nseg, slot0, F, reg, b.ws, op,
               (void *)stream), "completion segment");
  check_rc(gpu::complete_reduce(b.ws, b.mrow, b.mslot, m0, nm, slot0, F, reg,
                                op, (void *)stream), "completion reduce");
}

// out[p] = sum_f lam_f prod_t mats[t][inds[t,p], f]; inds is [nmodes, n]
static void py_gpu_kruskal_predict(Tensor inds, std::vector<Tensor> mats,
                                   py::object lam, Tensor out,
                                   int64_t stream) {
  const int64_t * base = dev_ptr<int64_t>(inds, "inds");
  double * op = dev_ptr<double>(out, "out");
  TORCH_CHECK(inds.dim() == 2, "inds must be [nmodes, n]");
  const size_t nm = (size_t)inds.size(0);
  const int64_t n = inds.size(1);
  TORCH_CHECK(nm >= 1 && nm <= 8 && mats.size() == nm,
              "need one factor per mode (1..8 modes)");
  TORCH_CHECK(out.numel() == n, "out length != number of coordinates");
  const int F = rank_of(mats);
  auto mp = factor_table<double>(mats, nm, F);
  const int64_t * ip[8] = {};
  for (size_t t = 0; t < nm; ++t) ip[t] = base + (int64_t)t * n;
  const double * lp = nullptr;
  Tensor lt;
  if (!lam.is_none()) {
    lt = lam.cast<Tensor>();
    lp = dev_ptr<double>(lt, "lam");
    TORCH_CHECK(lt.numel() == F, "lam length != rank");
  }
  check_rc(gpu::kruskal_predict(ip, mp.data(), (int)nm, lp, n, F, op,
                                (void *)stream), "kruskal_predict");
}

// One batch of the TTMc of a root-sorted stream: segments accumulate
// (single-segment rows go straight to `out`), then multi-segment rows are
// folded from `ws`. idx/mats are the non-root levels in level order; `out`
// is [rows, prod of their ranks] in that order; a slot is one output row.
static void py_gpu_ttmc(
    std::vector<Tensor> idx, std::vector<Tensor> mats, Tensor vals,
    Tensor seg_start, Tensor seg_len, Tensor seg_row, Tensor seg_slot,
    int64_t seg0, int64_t nseg, Tensor mrow, Tensor mslot, int64_t m0,
    int64_t nm, int64_t slot0, int64_t nslots, Tensor ws, Tensor out,
    int64_t stream) {
  const size_t nother = idx.size();
  TORCH_CHECK(nother >= 2 && nother <= 7, "ttmc supports 3..8 modes");
  const double * vp = dev_ptr<double>(vals, "vals");
  double * op = dev_ptr<double>(out, "out");
  TORCH_CHECK(out.dim() == 2, "out must be [rows, columns]");
  auto ip = stream_table(idx, nother, vals.numel());
  auto mp = ptr_table<double>(mats, nother, "factor");
  int ranks[8] = {};
  int64_t P = 1;
  for (size_t t = 0; t < nother; ++t) {
    TORCH_CHECK(mats[t].dim() == 2 && mats[t].size(1) >= 1
                && mats[t].size(1) <= 32,
                "ttmc supports rank 1..32 per mode, got ", mats[t].size(1));
    ranks[t] = (int)mats[t].size(1);
    P *= ranks[t];
  }
  TORCH_CHECK(P <= gpu::ttmc_max_cols(), "ttmc kernel supports at most ",
              gpu::ttmc_max_cols(), " output columns, got ", P);
  TORCH_CHECK(out.size(1) == P, "out has ", out.size(1), " columns, expected ",
              P);
  const SegBatch b(seg_start, seg_len, seg_row, seg_slot, seg0, nseg, mrow,
                   mslot, m0, nm, slot0, nslots, ws, P,
                   "ttmc workspace too small");
  check_rc(gpu::ttmc_segments(
               ip.data(), mp.data(), ranks, (int)nother, vp, b.seg_start,
               b.seg_len, b.seg_row, b.seg_slot, seg0, nseg, slot0, b.ws, op,
               (void *)stream), "ttmc segment");
  check_rc(gpu::ttmc_reduce(b.ws, b.mrow, b.mslot, m0, nm, slot0, (int)P, op,
                            (void *)stream), "ttmc reduce");
}

// --------------------------------------- Poisson CPD / CP-APR (f64 only)

// The multiplicative row update of one mode, up to max_inner inner
// iterations, no host synchronisation. Round 1 launches every segment
// (single-segment rows run all their iterations there) and the fold of the
// multi-segment rows; rounds 2..max_inner relaunch the multi-segment range
// and the fold. Segments [0, nsingle) have slot -1, the rest slots 0.. of
// `ws` (F doubles each); `done` (one flag per row) must come in zeroed.
static void py_hip_apr_update(
    std::vector<Tensor> idx, std::vector<Tensor> mats, Tensor vals,
    Tensor seg_start, Tensor seg_len, Tensor seg_row, Tensor seg_slot,
    int64_t nsingle, Tensor mrow, Tensor mslot, double eps_div,
    double inner_tol, int64_t max_inner, Tensor ws, Tensor done, Tensor B,
    Tensor Phi, Tensor iters, Tensor viol0, int64_t stream) {
  const size_t nother = idx.size();
  TORCH_CHECK(nother >= 2 && nother <= 7, "apr supports 3..8 modes");
  TORCH_CHECK(max_inner >= 1 && max_inner <= 0x7FFFFFFF,
              "max_inner must be >= 1");
  TORCH_CHECK(eps_div > 0.0, "eps_div must be > 0");
  const double * vp = dev_ptr<double>(vals, "vals");
  double * bp = dev_ptr<double>(B, "B");
  double * pp = dev_ptr<double>(Phi, "Phi");
  int32_t * itp = dev_ptr<int32_t>(iters, "iters");
  double * v0p = dev_ptr<double>(viol0, "viol0");
  int32_t * dp = dev_ptr<int32_t>(done, "done");
  TORCH_CHECK(B.dim() == 2, "B must be [rows, rank]");
  const int64_t rows = B.size(0);
  const int F = (int)B.size(1);
  TORCH_CHECK(F >= 1 && F <= 64, "apr supports rank 1..64, got ", F);
  TORCH_CHECK(Phi.dim() == 2 && Phi.size(0) == rows && Phi.size(1) == F,
              "Phi must have the shape of B");
  TORCH_CHECK(iters.numel() == rows && viol0.numel() == rows
              && done.numel() == rows,
              "iters, viol0 and done need one entry per row of B");
  auto ip = stream_table(idx, nother, vals.numel());
  auto mp = factor_table<double>(mats, nother, F);
  const int64_t nseg = seg_start.numel();
  const int64_t nm = mrow.numel();
  TORCH_CHECK(nsingle >= 0 && nsingle <= nseg, "nsingle out of range");
  const SegBatch b(seg_start, seg_len, seg_row, seg_slot, 0, nseg, mrow,
                   mslot, 0, nm, 0, nseg - nsingle, ws, F,
                   "apr workspace too small");
  void * st = (void *)stream;
  for (int round = 1; round <= (int)max_inner; ++round) {
    const int64_t seg0 = round == 1 ? 0 : nsingle;
    check_rc(gpu::apr_segments(
                 ip.data(), mp.data(), (int)nother, vp, b.seg_start,
                 b.seg_len, b.seg_row, b.seg_slot, seg0, nseg - seg0, F,
                 eps_div, inner_tol, (int)max_inner, dp, b.ws, bp, pp, itp,
                 v0p, st), "apr segment");
    check_rc(gpu::apr_fold(b.ws, b.mrow, b.mslot, nm, F, round, inner_tol,
                           (int)max_inner, dp, bp, pp, itp, v0p, st),
             "apr fold");
    if (nm == 0) break;
  }
}

// The damped-Newton (PDNR) row solve of one mode: one launch, one workgroup
// per entry of `rows` (the rows that have nonzeros, longest first), the
// whole inner loop of a row inside it, no host synchronisation. rowptr has
// one entry per row of B plus one; every output has one entry (Phi: one
// row) per row of B and comes in zeroed.
static void py_hip_apr_pdnr(
    std::vector<Tensor> idx, std::vector<Tensor> mats, Tensor vals,
    Tensor rowptr, Tensor rows, double eps_div, double inner_tol,
    int64_t max_inner, double mu0, Tensor B, Tensor Phi, Tensor iters,
    Tensor viol0, Tensor f0, Tensor f, Tensor mu, Tensor nback, Tensor nfail,
    int64_t stream) {
  const size_t nother = idx.size();
  TORCH_CHECK(nother >= 2 && nother <= 7, "apr supports 3..8 modes");
  TORCH_CHECK(max_inner >= 1 && max_inner <= 0x7FFFFFFF,
              "max_inner must be >= 1");
  TORCH_CHECK(eps_div > 0.0, "eps_div must be > 0");
  TORCH_CHECK(mu0 > 0.0, "mu0 must be > 0");
  const double * vp = dev_ptr<double>(vals, "vals");
  const int64_t * rp = dev_ptr<int64_t>(rowptr, "rowptr");
  const int32_t * rw = dev_ptr<int32_t>(rows, "rows");
  double * bp = dev_ptr<double>(B, "B");
  double * pp = dev_ptr<double>(Phi, "Phi");
  int32_t * itp = dev_ptr<int32_t>(iters, "iters");
  double * v0p = dev_ptr<double>(viol0, "viol0");
  double * f0p = dev_ptr<double>(f0, "f0");
  double * fp = dev_ptr<double>(f, "f");
  double * mup = dev_ptr<double>(mu, "mu");
  int32_t * nbp = dev_ptr<int32_t>(nback, "nback");
  int32_t * nfp = dev_ptr<int32_t>(nfail, "nfail");
  TORCH_CHECK(B.dim() == 2, "B must be [rows, rank]");
  const int64_t nrows = B.size(0);
  const int F = (int)B.size(1);
  TORCH_CHECK(F >= 1 && F <= 64, "apr supports rank 1..64, got ", F);
  TORCH_CHECK(Phi.dim() == 2 && Phi.size(0) == nrows && Phi.size(1) == F,
              "Phi must have the shape of B");
  TORCH_CHECK(iters.numel() == nrows && viol0.numel() == nrows
              && f0.numel() == nrows && f.numel() == nrows
              && mu.numel() == nrows && nback.numel() == nrows
              && nfail.numel() == nrows,
              "iters, viol0, f0, f, mu, nback and nfail need one entry per "
              "row of B");
  TORCH_CHECK(rowptr.numel() == nrows + 1,
              "rowptr needs one entry per row of B plus one");
  TORCH_CHECK(rows.numel() <= nrows, "more listed rows than rows of B");
  auto ip = stream_table(idx, nother, vals.numel());
  auto mp = factor_table<double>(mats, nother, F);
  check_rc(gpu::apr_pdnr(ip.data(), mp.data(), (int)nother, vp, rp, rw,
                         rows.numel(), F, eps_div, inner_tol, (int)max_inner,
                         mu0, bp, pp, itp, v0p, f0p, fp, mup, nbp, nfp,
                         (void *)stream), "apr pdnr");
}

// ------------------------------------- generalized CPD / GCP (f64 only)

// The loss-gradient pass of one mode: G[i] = sum dl/dm(val, mdl) pi over the
// stored entries of row i, and frow[i] = sum l(val, mdl) when frow is given.
// One launch of every segment and, if the plan has multi-segment rows, one
// fold; no host synchronisation. Segments [0, nsingle) have slot -1, the
// rest slots 0.. of `ws` (F doubles each, F + 1 with frow). G and frow must
// come in zeroed: rows without entries are not written.
static void py_hip_gcp_grad(
    std::vector<Tensor> idx, std::vector<Tensor> mats, Tensor vals,
    Tensor seg_start, Tensor seg_len, Tensor seg_row, Tensor seg_slot,
    int64_t nsingle, Tensor mrow, Tensor mslot, int64_t loss, double param,
    Tensor A, Tensor ws, Tensor G, py::object frow, int64_t stream) {
  const size_t nother = idx.size();
  TORCH_CHECK(nother >= 2 && nother <= 7, "gcp supports 3..8 modes");
  TORCH_CHECK(loss >= 0 && loss <= 7, "gcp loss id must be 0..7, got ", loss);
  TORCH_CHECK(loss != 1 || param > 0.0, "huber needs param > 0");
  const double * vp = dev_ptr<double>(vals, "vals");
  const double * ap = dev_ptr<double>(A, "A");
  double * gp = dev_ptr<double>(G, "G");
  TORCH_CHECK(A.dim() == 2, "A must be [rows, rank]");
  const int64_t rows = A.size(0);
  const int F = (int)A.size(1);
  TORCH_CHECK(F >= 1 && F <= 64, "gcp supports rank 1..64, got ", F);
  TORCH_CHECK(G.dim() == 2 && G.size(0) == rows && G.size(1) == F,
              "G must have the shape of A");
  double * fp = nullptr;
  Tensor ft;
  if (!frow.is_none()) {
    ft = frow.cast<Tensor>();
    fp = dev_ptr<double>(ft, "frow");
    TORCH_CHECK(ft.numel() == rows, "frow needs one entry per row of A");
  }
  auto ip = stream_table(idx, nother, vals.numel());
  auto mp = factor_table<double>(mats, nother, F);
  const int64_t nseg = seg_start.numel();
  const int64_t nm = mrow.numel();
  TORCH_CHECK(nsingle >= 0 && nsingle <= nseg, "nsingle out of range");
  const SegBatch b(seg_start, seg_len, seg_row, seg_slot, 0, nseg, mrow,
                   mslot, 0, nm, 0, nseg - nsingle, ws, F + (fp ? 1 : 0),
                   "gcp workspace too small");
  void * st = (void *)stream;
  check_rc(gpu::gcp_segments(
               ip.data(), mp.data(), (int)nother, vp, b.seg_start, b.seg_len,
               b.seg_row, b.seg_slot, nseg, F, (int)loss, param, ap, b.ws, gp,
               fp, st), "gcp segment");
  if (nm > 0)
    check_rc(gpu::gcp_fold(b.ws, b.mrow, b.mslot, nm, F, gp, fp, st),
             "gcp fold");
}

// ------------------------------------------- stochastic GCP (f64 only)

// The sampled-gradient pass: adds the semi-stratified estimate of every
// mode's gradient into grads (which come in zeroed) from the sample
// inds [nmodes, n] / vals [n], whose first p entries are stored draws.
// Returns the number of entries of `partials` that were written (their sum
// is the loss estimate), 0 without partials. Index VALUES are not checked:
// the caller guarantees inds[t] < mats[t].size(0).
static int64_t py_hip_sgcp_grad(Tensor inds, Tensor vals, int64_t p,
                                std::vector<Tensor> mats,
                                std::vector<Tensor> grads, int64_t loss,
                                double param, double wnz, double wz,
                                py::object partials, int64_t stream) {
  const int32_t * ip = dev_ptr<int32_t>(inds, "inds");
  const double * vp = dev_ptr<double>(vals, "vals");
  const size_t nm = mats.size();
  TORCH_CHECK(nm >= 3 && nm <= 8, "sgcp supports 3..8 modes");
  TORCH_CHECK(loss >= 0 && loss <= 7, "gcp loss id must be 0..7, got ", loss);
  TORCH_CHECK(loss != 1 || param > 0.0, "huber needs param > 0");
  const int64_t n = vals.numel();
  TORCH_CHECK(inds.dim() == 2 && inds.size(0) == (int64_t)nm
              && inds.size(1) == n, "inds must be [nmodes, p + q]");
  TORCH_CHECK(n >= 1 && p >= 0 && p <= n, "p out of range");
  const int F = rank_of(mats);
  TORCH_CHECK(F >= 1 && F <= 64, "sgcp supports rank 1..64, got ", F);
  auto mp = factor_table<double>(mats, nm, F);
  TORCH_CHECK(grads.size() == nm, "expected ", nm, " grads, got ",
              grads.size());
  std::array<double *, 8> gp{};
  for (size_t t = 0; t < nm; ++t) {
    gp[t] = dev_ptr<double>(grads[t], "grad");
    TORCH_CHECK(grads[t].sizes() == mats[t].sizes(),
                "grad ", t, " must have the shape of factor ", t);
    TORCH_CHECK(mats[t].size(0) <= 0x7FFFFFFF, "factor rows must fit int32");
  }
  double * pp = nullptr;
  int64_t nparts = 0;
  Tensor pt;
  if (!partials.is_none()) {
    pt = partials.cast<Tensor>();
    pp = dev_ptr<double>(pt, "partials");
    nparts = gpu::sgcp_nparts(n, (int)nm, F);
    TORCH_CHECK(pt.numel() >= nparts, "partials needs ", nparts,
                " entries, got ", pt.numel());
  }
  check_rc(gpu::sgcp_grad(ip, vp, n, p, mp.data(), gp.data(), (int)nm, F,
                          (int)loss, param, wnz, wz, pp, (void *)stream),
           "sgcp grad");
  return nparts;
}

// One fused Adam step on flat f64 buffers (launchers.hpp: adam_step).
static void py_hip_adam_step(Tensor x, Tensor g, Tensor m, Tensor v, double lr,
                             double beta1, double beta2, double eps, double c1,
                             double c2, c10::optional<double> lower,
                             int64_t stream) {
  double * xp = dev_ptr<double>(x, "x");
  double * gp = dev_ptr<double>(g, "g");
  double * mp = dev_ptr<double>(m, "m");
  double * vp = dev_ptr<double>(v, "v");
  const int64_t n = x.numel();
  TORCH_CHECK(x.dim() == 1 && g.dim() == 1 && m.dim() == 1 && v.dim() == 1
              && g.numel() == n && m.numel() == n && v.numel() == n,
              "x, g, m and v must be flat buffers of one length");
  TORCH_CHECK(xp != gp && xp != mp && xp != vp && gp != mp && gp != vp
              && mp != vp, "x, g, m and v must not alias");
  check_rc(gpu::adam_step(xp, gp, mp, vp, n, lr, beta1, beta2, eps, c1, c2,
                          lower.has_value(), lower.value_or(0.0),
                          (void *)stream), "adam step");
}

// ------------------------------------- constrained CPD / AO-ADMM (f64 only)

// The fused block-ADMM update of one factor: H and U are updated in place,
// iters receives one inner-iteration count per block of 64 rows.
static void py_gpu_admm_update(Tensor K, Tensor Ginv, Tensor rho, Tensor H,
                               Tensor U, Tensor iters, int64_t kind, double w,
                               double lo, double hi, double inner_tol,
                               int64_t max_inner, int64_t variant,
                               int64_t stream) {
  check_dev(K, torch::kFloat64, "K");
  check_dev(Ginv, torch::kFloat64, "Ginv");
  check_dev(rho, torch::kFloat64, "rho");
  check_dev(H, torch::kFloat64, "H");
  check_dev(U, torch::kFloat64, "U");
  check_dev(iters, torch::kInt32, "iters");
  TORCH_CHECK(H.dim() == 2, "H must be [rows, rank]");
  const int64_t n = H.size(0);
  const int F = (int)H.size(1);
  TORCH_CHECK(F >= 1 && F <= 64, "admm_update supports rank 1..64, got ", F);
  TORCH_CHECK(K.sizes() == H.sizes() && U.sizes() == H.sizes(),
              "K, H and U must have the same shape");
  TORCH_CHECK(Ginv.dim() == 2 && Ginv.size(0) == F && Ginv.size(1) == F,
              "Ginv must be [rank, rank]");
  TORCH_CHECK(rho.numel() == 1, "rho must have one element");
  TORCH_CHECK(iters.numel() == (n + 63) / 64,
              "iters must have one entry per block of 64 rows");
  TORCH_CHECK(kind >= 0 && kind <= 3, "unknown constraint kind ", kind);
  TORCH_CHECK(max_inner >= 0 && max_inner <= 0x7FFFFFFF,
              "max_inner out of range");
  TORCH_CHECK(variant == 0 || variant == 1
              || (variant == 2 && (F == 16 || F == 32 || F == 64)),
              "the MFMA variant exists for ranks 16, 32 and 64 only");
  check_rc(gpu::admm_update(
               K.data_ptr<double>(), Ginv.data_ptr<double>(),
               rho.data_ptr<double>(), H.data_ptr<double>(),
               U.data_ptr<double>(), iters.data_ptr<int32_t>(), n, F,
               (int)kind, w, lo, hi, inner_tol, (int)max_inner, (int)variant,
               (void *)stream), "admm_update");
}

// ------------------------------------------ fused dense ALS tail (f64 only)

// `inner` of the tail: [rank] when given
static double * inner_ptr(const c10::optional<Tensor> & inner, int F) {
  if (!inner.has_value()) return nullptr;
  double * p = dev_ptr<double>(*inner, "inner");
  TORCH_CHECK(inner->numel() == F, "inner must be [rank]");
  return p;
}

// One launch in front of the tail: Ginv = inverse of the Hadamard product
// of `grams` (+ reg on the diagonal) — none: Ginv is left alone — and the
// tail's accumulators reset: gram = 0, lam = 1, inner = 0 (when given).
static void py_gpu_als_prep(std::vector<Tensor> grams, double reg,
                            Tensor Ginv, Tensor gram, Tensor lam,
                            c10::optional<Tensor> inner, int64_t stream) {
  check_dev(Ginv, torch::kFloat64, "Ginv");
  check_dev(gram, torch::kFloat64, "gram");
  check_dev(lam, torch::kFloat64, "lam");
  TORCH_CHECK(Ginv.dim() == 2 && Ginv.size(0) == Ginv.size(1),
              "Ginv must be [rank, rank]");
  const int F = (int)Ginv.size(0);
  TORCH_CHECK(F >= 1 && F <= 64, "als_prep supports rank 1..64, got ", F);
  TORCH_CHECK(grams.size() <= 8, "at most 8 Gram matrices");
  TORCH_CHECK(gram.numel() == (int64_t)F * F && lam.numel() == F,
              "gram must be [rank, rank] and lam [rank]");
  auto gp = ptr_table<double>(grams, grams.size(), "grams");
  for (auto & g : grams) {
    TORCH_CHECK(g.numel() == (int64_t)F * F,
                "every Gram must be [rank, rank]");
    TORCH_CHECK(g.data_ptr() != gram.data_ptr(),
                "the Gram being reset cannot be an input");
  }
  check_rc(gpu::als_prep(gp.data(), (int)grams.size(), reg,
                         Ginv.data_ptr<double>(), F, gram.data_ptr<double>(),
                         lam.data_ptr<double>(), inner_ptr(inner, F),
                         (void *)stream),
           "als_prep", "als_prep kernel launch failed: bad arguments");
}

// The two passes of the tail. lam, gram and inner accumulate: they must
// have been reset by gpu_als_prep on the same stream.
static void py_gpu_als_tail(Tensor K, Tensor Ginv, Tensor A, Tensor lam,
                            Tensor gram, c10::optional<Tensor> inner,
                            int64_t stream) {
  check_dev(K, torch::kFloat64, "K");
  check_dev(Ginv, torch::kFloat64, "Ginv");
  check_dev(A, torch::kFloat64, "A");
  check_dev(lam, torch::kFloat64, "lam");
  check_dev(gram, torch::kFloat64, "gram");
  TORCH_CHECK(K.dim() == 2 && K.sizes() == A.sizes(),
              "K and A must be [rows, rank] of one shape");
  const int64_t n = K.size(0);
  const int F = (int)K.size(1);
  TORCH_CHECK(F == 16 || F == 32 || F == 64,
              "the fused tail exists for ranks 16, 32 and 64, got ", F);
  TORCH_CHECK(Ginv.numel() == (int64_t)F * F && gram.numel() == (int64_t)F * F
              && lam.numel() == F, "Ginv/gram must be [rank, rank], lam [rank]");
  TORCH_CHECK(K.data_ptr() != A.data_ptr(), "K and A must not alias");
  check_rc(gpu::als_tail(K.data_ptr<double>(), Ginv.data_ptr<double>(), n, F,
                         A.data_ptr<double>(), lam.data_ptr<double>(),
                         gram.data_ptr<double>(), inner_ptr(inner, F),
                         (void *)stream),
           "als_tail",
           "als_tail kernel launch failed: rank or alignment does not qualify");
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("gpu_als_prep", &py_gpu_als_prep,
        "Hadamard of Grams + SPD inverse + reset of the tail accumulators");
  m.def("gpu_als_tail", &py_gpu_als_tail,
        "fused ALS tail: A = (K Ginv)/lam, lam, gram += A^T A, inner");
  m.def("als_tail_cap_rows", &gpu::als_tail_cap_rows,
        "row count at which the fused tail's grid reaches its cap");
  m.def("gpu_admm_update", &py_gpu_admm_update,
        "fused block-ADMM factor update (in place on H, U)");
  m.def("hip_apr_update", &py_hip_apr_update,
        "CP-APR multiplicative row update of a root-sorted stream (f64)");
  m.def("hip_apr_pdnr", &py_hip_apr_pdnr,
        "CP-APR damped-Newton (PDNR) row solve of a root-sorted stream (f64)");
  m.def("hip_gcp_grad", &py_hip_gcp_grad,
        "GCP loss-gradient pass of a root-sorted stream (f64)");
  m.def("hip_sgcp_grad", &py_hip_sgcp_grad,
        "stochastic GCP: sampled gradient of every mode, atomics (f64)");
  m.def("hip_adam_step", &py_hip_adam_step,
        "fused Adam step on flat f64 buffers, g left zeroed");
  m.def("gpu_ttmc", &py_gpu_ttmc,
        "TTMc of a root-sorted stream: one batch of segments + row folds");
  m.def("ttmc_max_cols", &gpu::ttmc_max_cols,
        "widest TTMc output row the HIP kernel supports");
  m.def("gpu_complete_update", &py_gpu_complete_update,
        "row-wise completion update: one batch of segments + row solves");
  m.def("complete_slot_elems", &gpu::complete_slot_elems,
        "workspace doubles per segment slot at a rank");
  m.def("gpu_kruskal_predict", &py_gpu_kruskal_predict,
        "Kruskal model values at COO coordinates");
  m.def("tensor_load", &py_tensor_load, "load .tns/.bin tensor");
  m.def("tns_write", &py_tns_write);
  m.def("bin_write", &py_bin_write);
  m.def("coo_fix", &py_coo_fix, "sort+dedup and/or remove empty slices");
  m.def("csf_build", &py_csf_build, "CPU CSF build for a level permutation");
  m.def("mttkrp_stream", &py_mttkrp_stream, "COO gold-oracle MTTKRP (CPU)");
  m.def("mttkrp_csf_cpu", &py_mttkrp_csf, "CSF MTTKRP (CPU)");
  m.def("cpd_als_cpu", &py_cpd_als, "CPD-ALS on the CPU reference path");
  m.def("seeded_init", &py_seeded_init, "partition-invariant seeded factor init");
  m.def("order_modes", &py_order_modes, "CSF mode-order policies");
  m.def("gpu_mttkrp3", &py_gpu_mttkrp3, "3-mode CSF MTTKRP HIP kernels");
  m.def("gpu_mttkrp_flat", &py_gpu_mttkrp_flat,
        "flat expanded-CSF MTTKRP HIP kernel (3..5 modes)");
  m.def("gpu_mttkrp_flat_rp", &py_gpu_mttkrp_flat_rp,
        "flat MTTKRP with row pointers in place of the key stream (root "
        "output, key-sorted stream); false = declined, use gpu_mttkrp_flat");
  m.def("gpu_mttkrp_flat_v32", &py_gpu_mttkrp_flat_v32,
        "flat MTTKRP (v7) reading an f32 copy of f32-exact f64 values, by "
        "row pointers or key stream; false = declined, use the f64 stream");
  m.def("mttkrp_strip_gpu", &py_mttkrp_strip_gpu,
        "strip/window flat MTTKRP (root output in LDS tiles over a "
        "strip-layout stream); false = declined, use gpu_mttkrp_flat",
        py::arg("key"), py::arg("idx"), py::arg("mats"), py::arg("vals"),
        py::arg("s_row0"), py::arg("s_nrows"), py::arg("s_flags"),
        py::arg("s_bounds"), py::arg("tile_rows"), py::arg("wgs"),
        py::arg("out"), py::arg("stream"), py::arg("pace") = py::none(),
        py::arg("pace_us") = 2200, py::arg("slots") = py::none(),
        py::arg("ahead") = 0, py::arg("trace") = py::none());
  m.def("strip_wall_khz", &gpu::strip_wall_khz,
        "rate of the wall clock of the strip kernel's pace words, kHz");
  m.def("strip_wgs", &gpu::strip_wgs,
        "resident workgroups of a strip kernel instance on this device "
        "(rank, nother, f32 values, tile rows); 0 = no such instance");
  m.def("plan_strips", &py_plan_strips,
        "strips of a root-sorted stream: row0/nrows/flags/p0/p1 (host)");
  m.def("gpu_mttkrp_flat_det", &py_gpu_mttkrp_flat_det,
        "bitwise-deterministic flat MTTKRP (depth-0 streams, spec ranks)");
  m.def("flat_det_ws_elems", &gpu::flat_det_ws,
        "workspace elements required by gpu_mttkrp_flat_det");
  m.def("gpu_gram", &py_gpu_gram, "G += A^T A (tall-skinny, F<=64)");
  m.def("gpu_colacc", &py_gpu_colacc,
        "out[f] (pre-zeroed) += sum_i A[i,f]^2 (which=0), or "
        "out[f] = max(out[f], max_i |A[i,f]|) (which=1)");
  m.def("gpu_colscale", &py_gpu_colscale, "A[i,f] /= lam[f] in place");
  m.def("gpu_coldot", &py_gpu_coldot,
        "out[f] (pre-zeroed) += sum_i X[i,f] * A[i,f]");
  m.def("gpu_gram_det", &py_gpu_gram_det,
        "G = A^T A, per-block partials folded in fixed order "
        "(bitwise-deterministic)");
  m.def("gpu_rowsolve", &py_gpu_rowsolve,
        "C = A @ B (B is FxF, staged in LDS; bitwise-deterministic)");
  m.def("gpu_spd_inverse", &py_gpu_spd_inverse,
        "Ginv = G^-1 for SPD FxF (F<=64), one-workgroup Cholesky");
  m.def("gpu_mttkrp_flat5", &py_gpu_mttkrp_flat5,
        "LDS-staged flat MTTKRP (bucketed builds, root output)");
  m.def("gpu_mttkrp_flat6", &py_gpu_mttkrp_flat6,
        "LDS-staged flat MTTKRP over the packed int4 stream");
  m.def("gpu_mttkrp_det6", &py_gpu_mttkrp_det6,
        "LDS-staged deterministic MTTKRP (bucket-privatized outputs)");
  m.def("partition_weighted", [](std::vector<int64_t> w, int nparts) {
    int64_t bn = 0;
    auto parts = sp::partition_weighted(w.data(), (int64_t)w.size(), nparts, &bn);
    return py::make_tuple(parts, bn);
  }, "optimal chains-on-chains partition (boundaries, bottleneck)");
  m.def("hip_arch", &gpu::kernels_arch);
}
