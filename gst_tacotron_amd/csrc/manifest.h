// The named-tensor manifest of gsttaco.cpp: what a model (the main one, or a vocoder) expects to be loaded, by name and shape, and the
// host copies until finalize.  Host only; its own header so that a stand-alone program can exercise it (tools/manifest_check.cpp).
#pragma once
#include <stdint.h>

#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/gsttaco.h"

// Records msg as the context's last error (c == NULL: as the creation error) and returns code.  Defined by gsttaco.cpp.
int gt_fail(const gsttaco_ctx* c, int code, const std::string& msg);

struct HostTensor {
    std::string name;
    std::vector<int64_t> shape;
    std::vector<float> data;
    bool loaded = false;
    int64_t numel() const {
        int64_t n = 1;
        for (auto s : shape) n *= s;
        return n;
    }
};

struct Manifest {
    std::vector<HostTensor> tensors;
    std::map<std::string, int> index;

    void add(const std::string& name, std::vector<int64_t> shape) {
        HostTensor t;
        t.name = name;
        t.shape = std::move(shape);
        index[name] = (int)tensors.size();
        tensors.push_back(std::move(t));
    }
    // gsttaco_*_weight_info: tensor i's name, rank and shape (padded with 1 to four dimensions)
    int info(int i, const char** name, int64_t shape[4], int* ndim) const {
        if (i < 0 || i >= (int)tensors.size()) return GSTTACO_E_INVALID;
        const HostTensor& t = tensors[i];
        if (name) *name = t.name.c_str();
        if (ndim) *ndim = (int)t.shape.size();
        if (shape)
            for (size_t d = 0; d < 4; ++d) shape[d] = d < t.shape.size() ? t.shape[d] : 1;
        return 0;
    }
    // gsttaco_*_load_weight behind the caller's own checks: copies host into the tensor `name` when the shape is the manifest's.
    // prefix: what the model's messages start with ("" or "melgan: ").  A tensor may be loaded again; the last copy holds.
    int load(gsttaco_ctx* c, const char* prefix, const char* name, const float* host, const int64_t* shape, int ndim) {
        auto it = index.find(name);
        if (it == index.end()) return gt_fail(c, GSTTACO_E_WEIGHTS, std::string(prefix) + "unknown weight '" + name + "'");
        HostTensor& t = tensors[it->second];
        bool ok = ndim == (int)t.shape.size();
        for (int d = 0; ok && d < ndim; ++d) ok = shape[d] == t.shape[d];
        if (!ok) return gt_fail(c, GSTTACO_E_WEIGHTS, std::string(prefix) + "weight '" + name + "' has the wrong shape");
        t.data.assign(host, host + t.numel());
        t.loaded = true;
        return 0;
    }
    // the first tensor in manifest order that was never loaded, or NULL
    const HostTensor* first_unloaded() const {
        for (const HostTensor& t : tensors)
            if (!t.loaded) return &t;
        return nullptr;
    }
    const std::vector<float>& host(const std::string& name) const { return tensors[index.at(name)].data; }
};
