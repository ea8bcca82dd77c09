// cli.hpp -- the mechanics the host commands share: the clock, an argv cursor, the owner of the device context, the
// open / run / close wrapper around a command's output and a line reader for plain or gzipped text.  A command still owns
// its flag names, its value parsing, its messages and its usage text; nothing here knows a flag.  Header-only; the cursor
// and the reader need no device library (Device's members are only emitted where they are used).
#pragma once
#include <zlib.h>

#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../../include/goleft_depth.h"

namespace gdh {
namespace cli {

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// Walks argv[1..] word by word.  next() says what the word is; for a Flag, `key` is the part before '=' and `val` what
// followed it (has_val: there was an '=').  After `--` every word is a Positional, for the commands that honour it
// (terminator); for the others `--` is a Flag like any other word that starts with '-'.
class Args {
public:
    enum Kind { End, Help, Positional, Flag };
    std::string arg, key, val;                   // the word as written; its key; its value
    bool has_val = false;

    Args(int argc, const char* const* argv, void (*usage)(FILE*), bool terminator = true)
        : argc_(argc), argv_(argv), usage_(usage), terminator_(terminator) {}

    // Help: -h or --help, the usage is on stdout already
    Kind next()
    {
        if (++i_ >= argc_) return End;
        arg = argv_[i_];
        if (rest_) return Positional;
        if (arg == "-h" || arg == "--help") { usage_(stdout); return Help; }
        if (terminator_ && arg == "--") { rest_ = true; return next(); }
        if (arg.size() < 2 || arg[0] != '-') return Positional;
        const size_t eq = arg.find('=');
        has_val = eq != std::string::npos;
        key = arg.substr(0, eq);
        val = has_val ? arg.substr(eq + 1) : std::string();
        return Flag;
    }

    // the flag's value: what followed '=', else the next word; without one the error is printed and this is false
    bool value()
    {
        if (has_val) return true;
        if (i_ + 1 >= argc_) { fail("missing value for %s", key.c_str()); return false; }
        val = argv_[++i_];
        return true;
    }

    // "error: MESSAGE", then the usage, on stderr; -1 for the caller to return
    __attribute__((format(printf, 2, 3))) int fail(const char* fmt, ...) const
    {
        va_list ap;
        va_start(ap, fmt);
        fputs("error: ", stderr);
        vfprintf(stderr, fmt, ap);
        fputc('\n', stderr);
        va_end(ap);
        usage_(stderr);
        return -1;
    }

private:
    int argc_, i_ = 0;
    const char* const* argv_;
    void (*usage_)(FILE*);
    bool terminator_, rest_ = false;
};

// The device context of a command: destroyed when it goes out of scope, on every path.  Converts to the gd_ctx* the
// library calls take.
class Device {
public:
    Device() = default;
    Device(const Device&) = delete;
    Device& operator=(const Device&) = delete;
    ~Device() { reset(); }

    // the device GOLEFT_DEVICE names (default 0); false with the message printed in prog's name: the caller picks the code
    bool open(const char* prog)
    {
        int device = 0;
        if (const char* e = getenv("GOLEFT_DEVICE")) device = atoi(e);
        const int rc = gd_create(device, &ctx_);
        if (rc == GD_OK) return true;
        ctx_ = nullptr;
        fprintf(stderr, "%s: no usable MI355X device (%s); this build has no CPU path\n", prog, gd_strerror(rc));
        return false;
    }
    operator gd_ctx*() const { return ctx_; }
    void reset() { if (ctx_) gd_destroy(ctx_); ctx_ = nullptr; }     // destroy now: before the output is formatted
    void release() { ctx_ = nullptr; }                               // leave it to the exit of the process

private:
    gd_ctx* ctx_ = nullptr;
};

// fn(out) with out_path opened for writing, or stdout for null; a close that fails turns a 0 into 1
template <class Fn>
int run_to_output(const char* prog, const char* out_path, Fn fn)
{
    FILE* out = stdout;
    if (out_path && !(out = fopen(out_path, "w"))) { fprintf(stderr, "%s: cannot create %s\n", prog, out_path); return 1; }
    int r = fn(out);
    if (out_path) { if (fclose(out) != 0 && r == 0) r = 1; }
    else fflush(stdout);
    return r;
}

// The lines of a plain or gzipped file.
class Lines {
public:
    long long lineno = 0;                        // of the line next() gave last
    bool whole = false;                          // ... and whether it ended in a newline

    Lines() = default;
    Lines(const Lines&) = delete;
    Lines& operator=(const Lines&) = delete;
    ~Lines() { if (f_) gzclose(f_); }

    bool open(const std::string& path) { f_ = gzopen(path.c_str(), "rb"); return f_ != nullptr; }     // (a plain file is read as it is)

    // one line without its newline (and without a carriage return before it); false at the end of the file
    bool next(std::string* line)
    {
        line->clear();
        whole = false;
        char buf[1 << 16];
        bool any = false;
        while (gzgets(f_, buf, sizeof buf)) {
            any = true;
            const size_t n = strlen(buf);
            line->append(buf, n);
            if (n && buf[n - 1] == '\n') { whole = true; break; }
        }
        if (!any) return false;
        ++lineno;
        while (!line->empty() && (line->back() == '\n' || line->back() == '\r')) line->pop_back();
        return true;
    }

private:
    gzFile f_ = nullptr;
};

}  // namespace cli
}  // namespace gdh
