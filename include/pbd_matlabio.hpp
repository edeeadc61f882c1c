// pbd_matlabio.hpp -- pbdhost::MatlabIOModel: models in the layout the Matlab training code writes, read from a level 5
// MAT-file.  Header-only over zlib (link with -lz); the C++ twin of partsbaseddetector_amd/matio.py + matlab_model.py.
//
// It fills what pbdhost::FileStorageModel fills, by the conversions of the reference's MatlabIOModel::deserialize
// (src/MatlabIOModel.cpp:66-187): name (variable `name`, else the file stem), interval / thresh / sbin (truncated to
// int / rounded to float / truncated), norient = 18, filters(f).w (sizy x sizx x C) flattened to sizy x (sizx*C) with
// [m][n*C + c] = w(m, n, c), components{c}(p).filterid / defid / biasid / parent 0-based (index arrays row-major over
// Matlab's (i, j)), defs(d).w rounded to float, defs(d).anchor [x y ds] as Point(x - 1, y - 1) truncated, bias(b).w
// rounded to float.  Other fields are ignored; field order does not matter.
//
// MAT subset ("Matlab model files"): both byte orders, miCOMPRESSED, the small data element format,
// miMATRIX of the classes double, single, int8..64, uint8..64 (any numeric storage type; logical flag accepted), char, cell
// and struct, zero-byte (empty) miMATRIX.  Everything else -- v7.3 (HDF5) and level 4 files, sparse / complex / object / function handle /
// opaque arrays, and every malformed or truncated file -- is a pbdhost::Error(PBD_ERR_INVALID, ...).
#pragma once

#include <zlib.h>

#include "pbd_host.hpp"

namespace pbdhost {

class MatlabIOModel : public Model {
public:
    // one Matlab array; numbers are held as double (every field the model reads is converted to double first, as
    // cvmatio's find<double> / cv::Mat::at<double> do)
    struct Value {
        enum Kind { NUMERIC, CHAR, CELL, STRUCT };
        Kind kind;
        std::vector<size_t> dims;
        std::vector<double> num;            // NUMERIC: column-major
        std::string str;                    // CHAR: UTF-8
        std::vector<Value> items;           // CELL: linear order; STRUCT: element-major, then field
        std::vector<std::string> fields;    // STRUCT
        Value() : kind(NUMERIC) {}
        size_t count() const { size_t n = 1; for (size_t d = 0; d < dims.size(); ++d) n *= dims[d]; return n; }
    };

    bool deserialize(const std::string &filename)
    {   // src/MatlabIOModel.cpp:66-187
        std::ifstream in(filename.c_str(), std::ios::binary);
        if (!in) return false;
        std::vector<uint8_t> buf((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        file_ = filename;
        std::vector<std::pair<std::string, Value> > vars = read(buf);

        const Value *name = find(vars, "name");
        if (name) {
            if (name->kind != Value::CHAR) fail("variable name is not a char row");
            name_ = name->str;
        } else {
            std::string base = filename.substr(filename.find_last_of('/') == std::string::npos ? 0 : filename.find_last_of('/') + 1);
            const size_t dot = base.find_last_of('.');
            name_ = (dot == std::string::npos || dot == 0) ? base : base.substr(0, dot);
        }
        const Value *top = find(vars, "model");
        if (!top) fail("missing variable model");
        if (top->kind != Value::STRUCT || top->count() < 1) fail("model is not a struct array");
        const size_t root = 0;
        nscales_ = to_int(scalar(field(*top, root, "interval", "model"), "model.interval"), "model.interval");
        thresh_ = (float)scalar(field(*top, root, "thresh", "model"), "model.thresh");
        binsize_ = to_int(scalar(field(*top, root, "sbin", "model"), "model.sbin"), "model.sbin");
        norient_ = 18;

        filtersw_.clear();
        const Value &filters = structs(field(*top, root, "filters", "model"), "model.filters");
        for (size_t f = 0; f < filters.count(); ++f) {
            const std::string path = "model.filters(" + num_str(f + 1) + ")";
            const Value &w = numeric(field(filters, f, "w", path), path + ".w");
            if (w.dims.size() > 3) fail(path + ".w has more than 3 dimensions");
            const size_t M = w.dims[0], N = w.dims[1], C = w.dims.size() == 3 ? w.dims[2] : 1;
            flen_ = (int)C;
            MatT<double> flat((int)M, (int)(N * C));
            flat.data = row_major(w);                 // [m][n*C + c] = w(m, n, c)
            filtersw_.push_back(flat);
        }

        const Value &components = field(*top, root, "components", "model");
        if (components.kind != Value::CELL) fail("model.components is not a cell array");
        const size_t nc = components.items.size();
        parentid_.assign(nc, std::vector<int>());
        filterid_.assign(nc, std::vector<std::vector<int> >());
        biasid_ = filterid_; defid_ = filterid_;
        for (size_t c = 0; c < nc; ++c) {
            const std::string cpath = "model.components{" + num_str(c + 1) + "}";
            const Value &comp = structs(components.items[c], cpath);
            for (size_t p = 0; p < comp.count(); ++p) {
                const std::string path = cpath + "(" + num_str(p + 1) + ")";
                defid_[c].push_back(ids(field(comp, p, "defid", path), path + ".defid"));
                filterid_[c].push_back(ids(field(comp, p, "filterid", path), path + ".filterid"));
                parentid_[c].push_back(to_int(scalar(field(comp, p, "parent", path), path + ".parent"), path + ".parent") - 1);
                biasid_[c].push_back(ids(field(comp, p, "biasid", path), path + ".biasid"));
            }
        }

        defw_.clear();
        anchors_.clear();
        const Value &defs = structs(field(*top, root, "defs", "model"), "model.defs");
        for (size_t d = 0; d < defs.count(); ++d) {
            const std::string path = "model.defs(" + num_str(d + 1) + ")";
            const std::vector<double> w = row_major(numeric(field(defs, d, "w", path), path + ".w"));
            defw_.push_back(std::vector<float>(w.begin(), w.end()));
            const std::vector<double> a = row_major(numeric(field(defs, d, "anchor", path), path + ".anchor"));
            if (a.size() < 2) fail(path + ".anchor is not [x y ds]");
            anchors_.push_back(Point(to_int(a[0], path + ".anchor") - 1, to_int(a[1], path + ".anchor") - 1));
        }

        biasw_.clear();
        const Value &bias = structs(field(*top, root, "bias", "model"), "model.bias");
        for (size_t b = 0; b < bias.count(); ++b) {
            const std::string path = "model.bias(" + num_str(b + 1) + ")";
            biasw_.push_back((float)scalar(field(bias, b, "w", path), path + ".w"));
        }
        return true;
    }

private:
    std::string file_;

    void fail(const std::string &msg) const { throw Error(PBD_ERR_INVALID, "model file " + file_ + ": " + msg); }
    static std::string num_str(size_t v) { std::ostringstream s; s << v; return s.str(); }

    // ------------------------------------------------------------------ model-layout helpers
    static const Value *find(const std::vector<std::pair<std::string, Value> > &vars, const std::string &name)
    {
        for (size_t i = 0; i < vars.size(); ++i)
            if (vars[i].first == name) return &vars[i].second;
        return NULL;
    }
    const Value &field(const Value &s, size_t k, const std::string &name, const std::string &path) const
    {
        for (size_t f = 0; f < s.fields.size(); ++f)
            if (s.fields[f] == name) return s.items[k * s.fields.size() + f];
        fail("missing field " + path + "." + name);
        return s;
    }
    const Value &structs(const Value &v, const std::string &path) const
    {
        if (v.kind != Value::STRUCT) fail(path + " is not a struct array");
        return v;
    }
    const Value &numeric(const Value &v, const std::string &path) const
    {
        if (v.kind != Value::NUMERIC) fail(path + " is not a numeric array");
        return v;
    }
    double scalar(const Value &v, const std::string &path) const
    {
        if (numeric(v, path).num.empty()) fail(path + " is empty");
        return v.num[0];
    }
    int to_int(double x, const std::string &path) const
    {   // a double's conversion to int (truncation), refused where it is undefined
        if (!(x > -2147483648.0 && x < 2147483648.0)) fail(path + " is not an int");
        return (int)x;
    }
    static std::vector<double> row_major(const Value &v)
    {   // the logical index (i, j, k, ...) last-fastest: how cvmatio's cv::Mat (3rd dimension as channels) iterates
        std::vector<double> out;
        out.reserve(v.num.size());
        std::vector<size_t> idx(v.dims.size(), 0);
        for (size_t n = 0; n < v.num.size(); ++n) {
            size_t off = 0, stride = 1;
            for (size_t d = 0; d < v.dims.size(); ++d) { off += idx[d] * stride; stride *= v.dims[d]; }
            out.push_back(v.num[off]);
            for (size_t d = v.dims.size(); d-- > 0;) { if (++idx[d] < v.dims[d]) break; idx[d] = 0; }
        }
        return out;
    }
    std::vector<int> ids(const Value &v, const std::string &path) const
    {   // 1-based to 0-based
        const std::vector<double> a = row_major(numeric(v, path));
        std::vector<int> out;
        for (size_t i = 0; i < a.size(); ++i) out.push_back(to_int(a[i], path) - 1);
        return out;
    }

    // ------------------------------------------------------------------ MAT-file level 5
    enum { miINT8 = 1, miUINT8, miINT16, miUINT16, miINT32, miUINT32, miSINGLE, miDOUBLE = 9, miINT64 = 12, miUINT64,
           miMATRIX, miCOMPRESSED, miUTF8, miUTF16, miUTF32 };
    enum { mxCELL = 1, mxSTRUCT, mxOBJECT, mxCHAR, mxSPARSE, mxDOUBLE, mxSINGLE, mxINT8, mxUINT8, mxINT16, mxUINT16, mxINT32,
           mxUINT32, mxINT64, mxUINT64 };
    struct Elem {
        uint32_t type;
        const uint8_t *data;
        size_t n;
    };
    bool big_ = false;

    uint32_t u32(const uint8_t *p) const
    {
        return big_ ? ((uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3])
                    : ((uint32_t)p[3] << 24 | (uint32_t)p[2] << 16 | (uint32_t)p[1] << 8 | p[0]);
    }
    // the data element at buf[pos, end); pos moves to the next one
    Elem next(const uint8_t *buf, size_t &pos, size_t end, const std::string &where) const
    {
        if (pos > end || end - pos < 8) fail(where + ": truncated data element");
        Elem e;
        const uint32_t first = u32(buf + pos);
        if (first >> 16) {                    // small data element: type and size in one word, data in the next
            e.type = first & 0xFFFF;
            e.n = first >> 16;
            if (e.n > 4) fail(where + ": bad small data element");
            e.data = buf + pos + 4;
            pos += 8;
            return e;
        }
        e.type = first;
        e.n = u32(buf + pos + 4);
        const size_t start = pos + 8;
        if (e.n > end - start) fail(where + ": data element runs past the end of its container");
        e.data = buf + start;
        const size_t padded = e.type == miCOMPRESSED ? e.n : (e.n + 7) / 8 * 8;
        pos = padded > end - start ? end : start + padded;
        return e;
    }
    static size_t mi_size(uint32_t t)
    {
        switch (t) {
        case miINT8: case miUINT8: case miUTF8: return 1;
        case miINT16: case miUINT16: case miUTF16: return 2;
        case miINT32: case miUINT32: case miSINGLE: case miUTF32: return 4;
        case miDOUBLE: case miINT64: case miUINT64: return 8;
        default: return 0;
        }
    }
    double number(uint32_t t, const uint8_t *p) const
    {
        const size_t w = mi_size(t);
        uint8_t b[8];
        for (size_t i = 0; i < w; ++i) b[i] = big_ ? p[w - 1 - i] : p[i];   // to little-endian (the hosts this builds for)
        switch (t) {
        case miINT8: return (double)(int8_t)b[0];
        case miUINT8: return (double)b[0];
        case miINT16: { int16_t v; std::memcpy(&v, b, 2); return v; }
        case miUINT16: { uint16_t v; std::memcpy(&v, b, 2); return v; }
        case miINT32: { int32_t v; std::memcpy(&v, b, 4); return v; }
        case miUINT32: { uint32_t v; std::memcpy(&v, b, 4); return v; }
        case miSINGLE: { float v; std::memcpy(&v, b, 4); return v; }
        case miDOUBLE: { double v; std::memcpy(&v, b, 8); return v; }
        case miINT64: { int64_t v; std::memcpy(&v, b, 8); return (double)v; }
        default: { uint64_t v; std::memcpy(&v, b, 8); return (double)v; }
        }
    }
    std::vector<double> numbers(const Elem &e, const std::string &where) const
    {
        const size_t w = e.type == miUTF8 || e.type == miUTF16 || e.type == miUTF32 ? 0 : mi_size(e.type);
        if (!w) fail(where + ": data type " + num_str(e.type) + " is not numeric");
        if (e.n % w) fail(where + ": data size is not a whole number of values");
        std::vector<double> v(e.n / w);
        for (size_t i = 0; i < v.size(); ++i) v[i] = number(e.type, e.data + i * w);
        return v;
    }
    static void utf8(std::string &s, uint32_t c)
    {
        if (c < 0x80) s += (char)c;
        else if (c < 0x800) { s += (char)(0xC0 | c >> 6); s += (char)(0x80 | (c & 0x3F)); }
        else if (c < 0x10000) { s += (char)(0xE0 | c >> 12); s += (char)(0x80 | (c >> 6 & 0x3F)); s += (char)(0x80 | (c & 0x3F)); }
        else { s += (char)(0xF0 | (c >> 18 & 0x07)); s += (char)(0x80 | (c >> 12 & 0x3F)); s += (char)(0x80 | (c >> 6 & 0x3F)); s += (char)(0x80 | (c & 0x3F)); }
    }

    Value matrix(const uint8_t *buf, size_t n, const std::string &where_in, int depth) const
    {
        std::string where = where_in;
        if (depth > 64) fail(where + ": nested more than 64 levels deep");
        Value v;
        if (n == 0) { v.dims.assign(2, 0); return v; }           // zero-byte miMATRIX: an empty array
        size_t pos = 0;
        Elem flags = next(buf, pos, n, where);
        if (flags.type != miUINT32 || flags.n != 8) fail(where + ": bad array flags");
        const uint32_t word = u32(flags.data), cls = word & 0xFF;
        Elem dims = next(buf, pos, n, where);
        if (dims.type != miINT32 || dims.n < 8 || dims.n % 4) fail(where + ": bad dimensions");
        double total = 1;
        for (size_t i = 0; i < dims.n / 4; ++i) {
            const int32_t d = (int32_t)u32(dims.data + 4 * i);
            if (d < 0) fail(where + ": negative dimension");
            v.dims.push_back((size_t)d);
            total *= d;
        }
        if (total > (double)n * 8) fail(where + ": dimensions larger than the data");   // also bounds the count's product
        Elem name = next(buf, pos, n, where);
        if (name.type != miINT8) fail(where + ": bad array name");
        if (where.empty()) where = std::string((const char *)name.data, name.n);
        const size_t count = v.count();
        if (cls == mxCELL) {
            v.kind = Value::CELL;
            for (size_t k = 0; k < count; ++k) {
                const std::string sub = where + "{" + num_str(k + 1) + "}";
                Elem e = next(buf, pos, n, sub);
                if (e.type != miMATRIX) fail(sub + ": cell element is not an array");
                v.items.push_back(matrix(e.data, e.n, sub, depth + 1));
            }
        } else if (cls == mxSTRUCT) {
            v.kind = Value::STRUCT;
            Elem len = next(buf, pos, n, where);
            const std::vector<double> fl = len.type == miINT32 ? numbers(len, where) : std::vector<double>();
            if (fl.size() != 1 || fl[0] < 1) fail(where + ": bad struct field name length");
            const size_t L = (size_t)fl[0];
            Elem names = next(buf, pos, n, where);
            if (names.type != miINT8 || names.n % L) fail(where + ": bad struct field names");
            for (size_t i = 0; i < names.n; i += L) {
                const char *s = (const char *)names.data + i;
                v.fields.push_back(std::string(s, strnlen(s, L)));
            }
            for (size_t k = 0; k < count; ++k)
                for (size_t f = 0; f < v.fields.size(); ++f) {
                    const std::string sub = count == 1 ? where + "." + v.fields[f] : where + "(" + num_str(k + 1) + ")." + v.fields[f];
                    Elem e = next(buf, pos, n, sub);
                    if (e.type != miMATRIX) fail(sub + ": struct field is not an array");
                    v.items.push_back(matrix(e.data, e.n, sub, depth + 1));
                }
        } else if (cls == mxCHAR) {
            v.kind = Value::CHAR;
            if (pos < n) {
                Elem e = next(buf, pos, n, where);
                if (e.type == miUTF8 || e.type == miUINT8 || e.type == miINT8) {
                    if (e.type == miUTF8) v.str.assign((const char *)e.data, e.n);
                    else for (size_t i = 0; i < e.n; ++i) utf8(v.str, e.data[i]);
                } else if (e.type == miUINT16 || e.type == miINT16 || e.type == miUTF16 || e.type == miUINT32 ||
                           e.type == miINT32 || e.type == miUTF32) {
                    const size_t w = mi_size(e.type);
                    if (e.n % w) fail(where + ": bad character data");
                    for (size_t i = 0; i < e.n; i += w) utf8(v.str, w == 2 ? (uint32_t)number(miUINT16, e.data + i) : u32(e.data + i));
                } else {
                    fail(where + ": bad character data");
                }
            }
        } else if (cls >= mxDOUBLE && cls <= mxUINT64) {
            if (word & 0x0800) fail("variable " + where + ": complex data is not supported");
            Elem e = next(buf, pos, n, where);
            v.num = numbers(e, where);
            if (v.num.size() != count) fail(where + ": value count does not match the dimensions");
            if (cls == mxSINGLE) for (size_t i = 0; i < count; ++i) v.num[i] = (float)v.num[i];
        } else {
            static const char *names[] = {"", "cell", "struct", "object", "char", "sparse"};
            const std::string cname = cls <= mxSPARSE ? names[cls] : cls == 16 ? "function handle" : cls == 17 ? "opaque" : num_str(cls);
            fail("variable " + where + ": Matlab class " + cname + " is not supported");
        }
        return v;
    }

    std::vector<uint8_t> inflate_all(const uint8_t *p, size_t n) const
    {
        if (n > 0x7fffffffu) fail("compressed element too large");
        z_stream zs;
        std::memset(&zs, 0, sizeof zs);
        if (inflateInit(&zs) != Z_OK) fail("zlib initialisation failed");
        zs.next_in = const_cast<Bytef *>(p);
        zs.avail_in = (uInt)n;
        std::vector<uint8_t> out;
        int rc = Z_OK;
        while (rc != Z_STREAM_END) {
            const size_t have = out.size(), chunk = std::max<size_t>(1 << 16, have);
            if (have + chunk > ((size_t)1 << 31)) { inflateEnd(&zs); fail("compressed element inflates past 2 GiB"); }
            out.resize(have + chunk);
            zs.next_out = out.data() + have;
            zs.avail_out = (uInt)chunk;
            rc = inflate(&zs, Z_NO_FLUSH);
            out.resize(have + chunk - zs.avail_out);
            if (rc != Z_OK && rc != Z_STREAM_END) { inflateEnd(&zs); fail("corrupt or truncated compressed element"); }
            if (rc == Z_OK && zs.avail_in == 0 && zs.avail_out != 0) { inflateEnd(&zs); fail("truncated compressed element"); }
        }
        inflateEnd(&zs);
        return out;
    }

    std::vector<std::pair<std::string, Value> > read(const std::vector<uint8_t> &buf)
    {
        const std::string resave = "; re-save it in Matlab with save -v7";
        if (buf.size() < 4 || !buf[0] || !buf[1] || !buf[2] || !buf[3]) fail("not a MAT-file level 5 (a level 4 file, or not a MAT-file at all)" + resave);
        if (buf.size() < 128) fail("truncated MAT-file header");
        const std::string text((const char *)buf.data(), 116);
        if (text.find("MATLAB 7.3") != std::string::npos || (buf.size() >= 520 && !std::memcmp(&buf[512], "\x89HDF\r\n\x1a\n", 8)))
            fail("a v7.3 MAT-file is HDF5, which this reader does not read" + resave);
        if (buf[126] == 'I' && buf[127] == 'M') big_ = false;
        else if (buf[126] == 'M' && buf[127] == 'I') big_ = true;
        else fail("not a MAT-file level 5 (no endian indicator)" + resave);
        const unsigned version = big_ ? (buf[124] << 8 | buf[125]) : (buf[125] << 8 | buf[124]);
        if (version != 0x0100) fail("MAT-file version is not level 5" + resave);
        std::vector<std::pair<std::string, Value> > vars;
        size_t pos = 128;
        while (pos < buf.size()) {
            bool padding = buf.size() - pos < 8;
            for (size_t i = pos; padding && i < buf.size(); ++i) padding = !buf[i];
            if (padding) break;
            Elem e = next(buf.data(), pos, buf.size(), "top level");
            std::vector<uint8_t> inflated;
            if (e.type == miCOMPRESSED) {
                inflated = inflate_all(e.data, e.n);
                size_t ip = 0;
                e = next(inflated.data(), ip, inflated.size(), "compressed element");
            }
            if (e.type != miMATRIX || e.n == 0) fail("top-level data element is not a named array");
            Value v = matrix(e.data, e.n, "", 0);
            // the name, once more (matrix() used it only for messages)
            size_t p = 0;
            next(e.data, p, e.n, "");
            next(e.data, p, e.n, "");
            Elem name = next(e.data, p, e.n, "");
            vars.push_back(std::make_pair(std::string((const char *)name.data, name.n), v));
        }
        return vars;
    }
};

}  // namespace pbdhost
