// hmm_input.cpp -- what the decoders read: the stage that turns a .wav / .prd / .seq input into device symbols (`hmm scan`,
// `hmm segment` in all its forms, `hmm align`; its structs: hmm_host.h), the driver of the commands that work input by
// input, and the text files beside the inputs -- lines, fields, and the label files of `hmm transitions` and `hmm align`.
#include "hmm_host.h"

namespace e2hmm_host {

std::vector<std::string> split_on(const std::string& s, char sep)
{
    std::vector<std::string> out(1);
    for (char ch : s) {
        if (ch == sep) out.emplace_back();
        else out.back() += ch;
    }
    return out;
}

int read_lines(const char* path, std::vector<std::string>& lines)
{
    std::vector<unsigned char> bytes;
    if (read_file(path, bytes)) return 1;
    lines = split_on(std::string(bytes.begin(), bytes.end()), '\n');
    for (std::string& l : lines)
        if (!l.empty() && l.back() == '\r') l.pop_back();
    while (!lines.empty() && lines.back().empty()) lines.pop_back();
    return 0;
}

int read_label_file(const char* path, std::vector<LabelRow>& rows)
{
    std::vector<std::string> lines;
    if (read_lines(path, lines)) return 1;
    // the first line that is no '#' comment is the header: a segment CSV (column `class`) or a tab-separated selection table
    size_t h = 0;
    while (h < lines.size() && (lines[h].empty() || lines[h][0] == '#')) ++h;
    if (h == lines.size()) return e2vq_set_error("%s: no header", path);
    const bool table = lines[h].find('\t') != std::string::npos;
    const std::vector<std::string> head = split_on(lines[h], table ? '\t' : ',');
    auto column = [&](const char* name) { return (int)(std::find(head.begin(), head.end(), name) - head.begin()); };
    const int ncol = (int)head.size();
    const int c_label = column(table ? "Type" : "class"), c_time = table ? column("Begin Time (s)") : -1;
    if (c_label == ncol || c_time == ncol)
        return e2vq_set_error("%s:%zu: neither a segment CSV (column 'class') nor a selection table (tab-separated, 'Begin Time (s)' and 'Type')",
                              path, h + 1);
    std::vector<std::pair<double, LabelRow>> timed;  // (begin time or row number, label)
    for (size_t l = h + 1; l < lines.size(); ++l) {
        if (lines[l].empty() || lines[l][0] == '#') continue;
        const std::vector<std::string> cells = split_on(lines[l], table ? '\t' : ',');
        if ((int)cells.size() != ncol) return e2vq_set_error("%s:%zu: %zu fields, not %d", path, l + 1, cells.size(), ncol);
        double at = (double)timed.size();
        if (table) {
            char* end = nullptr;
            at = strtod(cells[(size_t)c_time].c_str(), &end);
            if (cells[(size_t)c_time].empty() || *end || std::isnan(at))
                return e2vq_set_error("%s:%zu: begin time '%s' is not a number", path, l + 1, cells[(size_t)c_time].c_str());
        }
        timed.emplace_back(at, LabelRow{cells[(size_t)c_label], l + 1});
    }
    std::stable_sort(timed.begin(), timed.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    rows.clear();
    for (auto& r : timed) rows.push_back(std::move(r.second));
    return 0;
}

// ---- input -> device symbols ------------------------------------------------------------------------------------------------
int sym_inputs_check(const char* who, int M, const char* cb_filename, const char* const* input_filenames, int num_inputs,
                            int P, int W_ms, int O_ms, const char* csv_dir_or_file, SymInputs& si)
{
    si.have_cb = cb_filename && *cb_filename;
    if (si.have_cb) {
        char cls[96];
        if (e2vq_cbook_info(cb_filename, cls, &si.cbP, &si.cbM)) return 1;
        if (si.cbM != M) return e2vq_set_error("%s: codebook has M=%d but the models have M=%d", cb_filename, si.cbM, M);
    }
    const bool have_cb = si.have_cb;
    const int cbP = si.cbP;
    std::vector<SymInput>& inputs = si.inputs;
    inputs.assign((size_t)num_inputs, SymInput());
    const std::string csv = csv_dir_or_file ? csv_dir_or_file : "";
    const bool csv_is_file = num_inputs == 1 && ends_with(csv, ".csv");
    for (int f = 0; f < num_inputs; ++f) {
        SymInput& in = inputs[(size_t)f];
        if (!input_filenames[f]) return e2vq_set_error("%s: NULL file name", who);
        in.path = input_filenames[f];
        char cls[96];
        if (ends_with(in.path, ".seq")) {
            in.kind = 2;
            int m;
            if (e2vq_seq_info(in.path.c_str(), cls, &m, &in.T)) return 1;
            if (m != M) return e2vq_set_error("%s: codebook size %d differs from the models' %d", in.path.c_str(), m, M);
        } else if (ends_with(in.path, ".prd")) {
            in.kind = 1;
            int p;
            if (e2vq_prd_info(in.path.c_str(), cls, &p, &in.T)) return 1;
            if (have_cb && p != cbP)
                return e2vq_set_error("%s: prediction order %d differs from the codebook's %d", in.path.c_str(), p, cbP);
            si.need_cb = true;
        } else if (ends_with(in.path, ".wav")) {
            in.kind = 0;
            if (e2vq_wav_info(in.path.c_str(), &in.sample_rate, &in.samples, nullptr)) return 1;
            if (have_cb && P != cbP) return e2vq_set_error("%s: prediction order -P %d differs from the codebook's %d", in.path.c_str(), P, cbP);
            int win, off;
            if (e2vq_lpc_frame_count(in.samples, in.sample_rate, W_ms, O_ms, &win, &off, &in.T)) return 1;
            if (in.T < 0) return e2vq_set_error("%s: signal too short (%lld samples, window %d)", in.path.c_str(), (long long)in.samples, win);
            si.need_cb = true;
        } else {
            return e2vq_set_error("%s: not a .wav, .prd or .seq file", in.path.c_str());
        }
        if (!csv.empty()) in.csv = csv_is_file ? csv : csv + "/" + e2vq_io::basename_noext(in.path.c_str()) + ".csv";
        for (int g = 0; g < f && !in.csv.empty(); ++g)
            if (inputs[(size_t)g].csv == in.csv) return e2vq_set_error("%s and %s would both write %s", inputs[(size_t)g].path.c_str(), in.path.c_str(), in.csv.c_str());
    }
    if (si.need_cb && !have_cb) return e2vq_set_error("%s: signals and predictors need a codebook", who);
    if (si.need_cb) {
        si.refl.resize((size_t)si.cbM * (cbP + 1));
        if (e2vq_cbook_read(cb_filename, si.refl.data(), si.cbM)) return 1;
    }
    return 0;
}

int SymStage::open(int device_, const SymInputs& si)
{
    device = device_;
    if (st.create()) return 1;
    if (!si.need_cb) return 0;
    return e2vq_session_create(device, si.cbP, &vq.s) || e2vq_set_stream(vq.s, (void*)st.s) || e2vq_set_codebook(vq.s, si.refl.data(), si.cbM);
}

int SymStage::input(const SymInput& in, const SymInputs& si, int P, int W_ms, int O_ms, int64_t* T_out)
{
    const hipStream_t stream = st.s;
    const int cbP = si.cbP, NC = cbP + 1;
    int64_t T = in.T;
    std::vector<uint16_t> h_sym;
    std::vector<double> h_frames;
    if (in.kind == 2) {
        h_sym.resize((size_t)std::max<int64_t>(T, 1));
        if (T > 0 && e2vq_seq_read(in.path.c_str(), h_sym.data(), T)) return 1;
        if (d_sym.upload(h_sym.data(), (size_t)T, stream)) return 1;
        HIPCHK(hipStreamSynchronize(stream));  // (`h_sym` is a local)
    } else {
        if (d_frames.reserve((size_t)std::max<int64_t>(T, 1) * NC) || d_sym.reserve((size_t)T + 64)) return 1;
        if (in.kind == 1) {
            h_frames.resize((size_t)std::max<int64_t>(T, 1) * NC);
            bool fin = true;
            if (T > 0 && e2vq_io::prd_read_range_mt(in.path.c_str(), cbP, 0, T, h_frames.data(), e2vq_io::io_threads(), &fin)) return 1;
            if (!fin) return e2vq_set_error("%s: contains NaN or infinite values", in.path.c_str());
            if (T > 0) HIPCHK(hipMemcpyAsync(d_frames.get(), h_frames.data(), (size_t)T * NC * 8, hipMemcpyHostToDevice, stream));
        } else {
            std::vector<int32_t> samples((size_t)std::max<int64_t>(in.samples, 1));
            if (e2vq_wav_read(in.path.c_str(), samples.data(), in.samples)) return 1;
            if (d_status.reserve((size_t)std::max<int64_t>(T, 1))) return 1;
            int64_t T2 = 0;
            if (T > 0 && e2vq_lpc_analyze(device, P, W_ms, O_ms, samples.data(), in.samples, in.sample_rate, d_frames.get(),
                                          d_status.get(), T, &T2, 1))
                return 1;
            std::vector<int32_t> fst((size_t)T);
            if (T > 0) HIPCHK(hipMemcpyAsync(fst.data(), d_status.get(), (size_t)T * 4, hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
            int64_t good = 0;
            for (int64_t t = 0; t < T; ++t) good += fst[(size_t)t] == 0;
            if (good != T) {
                // frames whose Levinson recursion failed are left out, as `ecoz2 lpc` leaves them out of the .prd: the rest
                // makes one round trip through the host (the only place where the frames leave the device)
                h_frames.resize((size_t)T * NC);
                HIPCHK(hipMemcpy(h_frames.data(), d_frames.get(), (size_t)T * NC * 8, hipMemcpyDeviceToHost));
                int64_t o = 0;
                for (int64_t t = 0; t < T; ++t)
                    if (fst[(size_t)t] == 0) memmove(h_frames.data() + (size_t)(o++) * NC, h_frames.data() + (size_t)t * NC, (size_t)NC * 8);
                printf("%s: %lld frames left out: Levinson status != 0 (later frame times are early by their offsets)\n",
                       in.path.c_str(), (long long)(T - good));
                T = good;
                if (T > 0) HIPCHK(hipMemcpyAsync(d_frames.get(), h_frames.data(), (size_t)T * NC * 8, hipMemcpyHostToDevice, stream));
            }
        }
        if (T > 0 && e2vq_quantize_device(vq.s, d_frames.get(), T, d_sym.get(), nullptr)) return 1;
        HIPCHK(hipStreamSynchronize(stream));  // (`h_frames` is a local)
    }
    *T_out = T;
    return 0;
}

int SymStage::gather(const char* who, const SymInputs& si, int P, int W_ms, int O_ms, DeviceBuffer<unsigned short>& d_all,
                     std::vector<i64>& offs)
{
    // (the frame counts known so far bound the buffer: a .wav may still lose frames)
    i64 room = 0;
    for (const SymInput& in : si.inputs) room += in.T;
    if (d_all.reserve((size_t)room)) return 1;
    offs.assign(1, 0);
    for (const SymInput& in : si.inputs) {
        int64_t T = 0;
        if (input(in, si, P, W_ms, O_ms, &T)) return 1;
        if (offs.back() + T > room) return e2vq_set_error("%s: internal error: %s gave more frames than its header counts", who, in.path.c_str());
        // (on the stage's stream: the next input overwrites d_sym only behind this copy)
        if (T > 0) HIPCHK(hipMemcpyAsync(d_all.get() + offs.back(), d_sym.get(), (size_t)T * 2, hipMemcpyDeviceToDevice, st.s));
        offs.push_back(offs.back() + T);
    }
    return 0;
}

int run_on_files(const char* who, int M, const char* cb_filename, const char* const* input_filenames, int num_inputs, int P, int W_ms,
                 int O_ms, const char* csv_dir_or_file,
                 const std::function<int(const SymInput&, int64_t, const unsigned short*, hipStream_t)>& run)
{
    SymInputs si;
    if (sym_inputs_check(who, M, cb_filename, input_filenames, num_inputs, P, W_ms, O_ms, csv_dir_or_file, si)) return 1;
    // ---- the device from here on --------------------------------------------------------------------------------
    const int device = env_device();
    SymStage stg;
    if (require_device(device) || stg.open(device, si)) return 1;
    for (const SymInput& in : si.inputs) {
        int64_t T = 0;
        if (stg.input(in, si, P, W_ms, O_ms, &T)) return 1;
        if (run(in, T, stg.d_sym.get(), stg.st.s)) return 1;
    }
    return 0;
}

}  // namespace e2hmm_host
