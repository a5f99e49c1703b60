// m2t_layout.h -- the layout table every plan of the C ABI holds (m2t_plan, m2t_swin, m2t_text): the flat parameter
// inventory, the packed-weight region, the optional fp32 side region, named workspace regions, and the query keys that
// read them.  Host code only.  Names are for m2t_*_create and m2t_*_query: every handle resolves them to plain offsets once, as
// it registers them (m2t_plan_handles of m2t_api.hip, the tower handles of m2t_tower.h), and its passes look nothing up.
#pragma once
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#define CK(call) do { int rc__ = (call); if (rc__) return rc__; } while (0)

// named tensors of one device buffer, each aligned to 256 bytes
struct m2t_region {
  struct Tensor { size_t off, n; };          // byte offset, element count
  std::map<std::string, Tensor> t;
  size_t bytes = 0;
  size_t add(const std::string& name, size_t elems, size_t es) {
    bytes = (bytes + 255) & ~(size_t)255;
    t[name] = Tensor{bytes, elems};
    bytes += elems * es;
    return t[name].off;
  }
  void seal() { bytes = (bytes + 255) & ~(size_t)255; }
  void clear() { t.clear(); bytes = 0; }
};

struct m2t_layout {
  size_t esz = 4;                                   // bytes of the plan's element type T
  std::vector<std::string> pnames;                  // parameters in flat order; offsets and counts in floats
  std::map<std::string, long long> poff, pnum;
  long long nparams = 0;
  std::map<std::string, long long> pk;              // packed weights: offsets in elements of T, 8-element aligned, inside ws "packed"
  long long npacked = 0;
  std::map<std::string, long long> fb;              // fp32 side region (fused biases): offsets in floats
  long long nfb = 0;
  m2t_region ws;

  long long add_param(const std::string& n, long long cnt) { pnames.push_back(n); poff[n] = nparams; pnum[n] = cnt; nparams += cnt; return nparams - cnt; }
  long long add_pack(const std::string& n, long long cnt) {
    npacked = (npacked + 7) & ~7LL;
    pk[n] = npacked;
    npacked += cnt;
    return pk[n];
  }
  long long add_fb(const std::string& n, long long cnt) { fb[n] = nfb; nfb += cnt; return nfb - cnt; }
  const char* param_name(int i) const { return (i < 0 || i >= (int)pnames.size()) ? nullptr : pnames[i].c_str(); }

  // the generic keys; `families` names the name-keyed families beyond param: / numel: this handle answers (anything else: -1)
  enum { Q_WS = 1, Q_WSN = 2, Q_PACKED = 4 };
  long long query(const std::string& k, unsigned families) const {
    auto find = [&k](const std::map<std::string, long long>& m, size_t prefix) {
      auto it = m.find(k.substr(prefix));
      return it == m.end() ? -1 : it->second;
    };
    if (k == "workspace_bytes") return (long long)ws.bytes;
    if (k == "num_params") return nparams;
    if (k == "num_param_tensors") return (long long)pnames.size();
    if (k.rfind("param:", 0) == 0) return find(poff, 6);
    if (k.rfind("numel:", 0) == 0) return find(pnum, 6);
    if ((families & Q_WS) && k.rfind("ws:", 0) == 0) { auto it = ws.t.find(k.substr(3)); return it == ws.t.end() ? -1 : (long long)it->second.off; }
    if ((families & Q_WSN) && k.rfind("wsn:", 0) == 0) { auto it = ws.t.find(k.substr(4)); return it == ws.t.end() ? -1 : (long long)it->second.n; }
    if ((families & Q_PACKED) && k.rfind("packed:", 0) == 0) return find(pk, 7);
    return -1;
  }
};
