// Python bindings for the sonata_amd CDNA4 kernel library + the C++
// VitsEngine runtime.
#include <torch/extension.h>

#include "engine/vits_engine.h"

// elementwise.hip
torch::Tensor layer_norm_ct(torch::Tensor x, c10::optional<torch::Tensor> res,
                            torch::Tensor gamma, torch::Tensor beta,
                            double eps);
torch::Tensor fused_gate(torch::Tensor x, c10::optional<torch::Tensor> g,
                         long n_channels);
torch::Tensor fused_gate_cl(torch::Tensor x, c10::optional<torch::Tensor> g,
                            long n_channels);
torch::Tensor prior_sample(torch::Tensor m, torch::Tensor logs,
                           torch::Tensor mask, torch::Tensor noise,
                           double noise_scale);
torch::Tensor expand_states(torch::Tensor stats, torch::Tensor durs,
                            long F_max);
torch::Tensor mask_tail_(torch::Tensor x, torch::Tensor lens);
torch::Tensor seeded_noise(long B, long C, long T_max, torch::Tensor lens,
                           torch::Tensor seeds, torch::ScalarType dtype);
torch::Tensor row_ln_cl(torch::Tensor x, c10::optional<torch::Tensor> resid,
                        torch::Tensor gamma, torch::Tensor beta, double eps);
torch::Tensor depthwise_cl(torch::Tensor x, torch::Tensor w,
                           c10::optional<torch::Tensor> bias, long dil,
                           long pad);
torch::Tensor wn_step(torch::Tensor h, c10::optional<torch::Tensor> output,
                      torch::Tensor rs, torch::Tensor mc, long layer);
std::vector<torch::Tensor> flow_split_rev(torch::Tensor xc);
std::vector<torch::Tensor> coupling_tail(torch::Tensor x0, torch::Tensor x1,
                                         torch::Tensor post, torch::Tensor mc,
                                         bool last);
std::vector<torch::Tensor> dds_sep_ln_gelu(
    torch::Tensor x, c10::optional<torch::Tensor> g, torch::Tensor mc,
    torch::Tensor w, torch::Tensor bias, torch::Tensor gamma,
    torch::Tensor beta, long dil, double eps);
torch::Tensor ln_gelu_add(torch::Tensor y, torch::Tensor t, torch::Tensor mc,
                          torch::Tensor gamma, torch::Tensor beta,
                          bool last, double eps);
torch::Tensor spline_tail(torch::Tensor inputs, torch::Tensor cumwidths,
                          torch::Tensor cumheights, torch::Tensor derivatives,
                          double tail_bound);
torch::Tensor prior_sample_rows(torch::Tensor m, torch::Tensor logs,
                                torch::Tensor mask, torch::Tensor noise,
                                torch::Tensor noise_scale);
torch::Tensor scale_mask_rows(torch::Tensor noise, torch::Tensor mask,
                              torch::Tensor scales);
std::vector<torch::Tensor> duration_rows(torch::Tensor logw,
                                         torch::Tensor x_mask,
                                         torch::Tensor length_scale);
// conv1d.hip
torch::Tensor conv1d_fused(torch::Tensor x, torch::Tensor w_perm,
                           c10::optional<torch::Tensor> bias, long Cout,
                           long k, long stride, long padding, long dilation,
                           long groups, double pre_lrelu, long act_mode,
                           double post_slope,
                           c10::optional<torch::Tensor> residual);
torch::Tensor convtranspose1d_fused(torch::Tensor x, torch::Tensor w_perm,
                                    c10::optional<torch::Tensor> bias,
                                    long Cout, long k, long stride,
                                    long padding, double pre_lrelu);
// conv1d_cl.hip (channel-last)
torch::Tensor conv1d_cl_fused(torch::Tensor x, torch::Tensor w_perm,
                              c10::optional<torch::Tensor> bias, long Cout,
                              long k, long padding, long dilation,
                              double pre_lrelu, long act_mode,
                              double post_slope,
                              c10::optional<torch::Tensor> residual,
                              c10::optional<torch::Tensor> out_lens);
torch::Tensor convtranspose1d_cl_fused(torch::Tensor x, torch::Tensor w_perm,
                                       c10::optional<torch::Tensor> bias,
                                       long Cout, long k, long stride,
                                       long padding, double pre_lrelu,
                                       c10::optional<torch::Tensor> out_lens);
torch::Tensor conv1d_cl_wdirect(torch::Tensor x, torch::Tensor w_perm,
                                c10::optional<torch::Tensor> bias, long Cout,
                                long k, long padding, long dilation,
                                double pre_lrelu, long act_mode,
                                double post_slope,
                                c10::optional<torch::Tensor> residual,
                                c10::optional<torch::Tensor> out_lens);
torch::Tensor conv1d_direct_cl(torch::Tensor x, torch::Tensor w_perm,
                               c10::optional<torch::Tensor> bias, long Cout,
                               long k, long padding, long dilation,
                               double pre_lrelu, long act_mode,
                               double post_slope,
                               c10::optional<torch::Tensor> residual,
                               c10::optional<torch::Tensor> out_lens);
// attention_cl.hip
torch::Tensor attn_relpos_cl(torch::Tensor qkv, torch::Tensor rel_k,
                             torch::Tensor rel_v,
                             c10::optional<torch::Tensor> lens, long H,
                             long window, double scale);
// resblock_cl.hip
torch::Tensor resblock_pair_cl_fused(torch::Tensor x, torch::Tensor w1_perm,
                                     torch::Tensor b1, torch::Tensor w2_perm,
                                     torch::Tensor b2, long k, long dil,
                                     c10::optional<torch::Tensor> out_lens,
                                     c10::optional<torch::Tensor> accum,
                                     double out_scale);
bool resblock_wlayout_sliced(long CP);
torch::Tensor resblock_pair_cl_fused_sliced(
    torch::Tensor x, torch::Tensor w1_sliced, torch::Tensor b1,
    torch::Tensor w2_sliced, torch::Tensor b2, long k, long dil,
    c10::optional<torch::Tensor> out_lens, c10::optional<torch::Tensor> accum,
    double out_scale);
torch::Tensor resblock_chain_cl_fused(
    torch::Tensor x, torch::Tensor w_all, torch::Tensor b_all, long k,
    long d1, long d2, long d3, c10::optional<torch::Tensor> out_lens,
    c10::optional<torch::Tensor> accum, double out_scale);
// prosody.hip
torch::Tensor resample_linear_rows(torch::Tensor x, torch::Tensor in_len,
                                   torch::Tensor out_len, long N_out_max);
torch::Tensor scale_rows(torch::Tensor x, torch::Tensor len,
                         torch::Tensor gain);
std::vector<torch::Tensor> wsola_rows(torch::Tensor x, torch::Tensor in_len,
                                      torch::Tensor ana_hop,
                                      torch::Tensor n_frames,
                                      torch::Tensor out_len,
                                      torch::Tensor window, long half,
                                      long search, torch::Tensor gain,
                                      long N_out_max, long K_max);
std::vector<torch::Tensor> wsola_stream_rows(
    torch::Tensor x, std::vector<int64_t> par, std::vector<double> hop,
    std::vector<double> gain, torch::Tensor carry, torch::Tensor tails,
    torch::Tensor window, long half, long search, long N_out, long K_max);
torch::Tensor resample_stream_rows(torch::Tensor x, std::vector<int64_t> par,
                                   torch::Tensor carry, long N_out);
// pcm.hip
std::vector<torch::Tensor> pcm16_rows(torch::Tensor x, torch::Tensor len,
                                      long N_out, bool peak_normalize);
long pcm_tile();
std::vector<torch::Tensor> g711_rows(torch::Tensor x, torch::Tensor len,
                                     torch::Tensor law, long N_out,
                                     bool peak_normalize);
// resample.hip
torch::Tensor resample_poly_rows(torch::Tensor x, torch::Tensor in_len,
                                 torch::Tensor out_len, torch::Tensor bank,
                                 long L, long M, long H, long n_out);
torch::Tensor resample_poly_stream_rows(torch::Tensor x,
                                        std::vector<int64_t> par,
                                        torch::Tensor state,
                                        torch::Tensor bank, long L, long M,
                                        long H, long n_out);
long resample_tile();
// stream.hip
torch::Tensor gather_windows(std::vector<torch::Tensor> zs,
                             std::vector<int64_t> src,
                             std::vector<int64_t> row,
                             std::vector<int64_t> start,
                             std::vector<int64_t> length, long l_max);
torch::Tensor stream_seam_rows(torch::Tensor wav, std::vector<int64_t> lo,
                               std::vector<int64_t> hi,
                               std::vector<int64_t> ext,
                               std::vector<int64_t> prev_ext,
                               std::vector<int64_t> slot,
                               torch::Tensor tails_in,
                               torch::Tensor tails_out, torch::Tensor ramp,
                               long n_out);
long seam_crossfade_samples();

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "sonata_amd hand-written CDNA4 (gfx950) kernels";
  m.def("layer_norm_ct", &layer_norm_ct, "LayerNorm over channels of [B,C,T]");
  m.def("fused_gate", &fused_gate, "WaveNet tanh*sigmoid gate");
  m.def("fused_gate_cl", &fused_gate_cl, "channel-last WaveNet gate");
  m.def("prior_sample", &prior_sample, "z=(m+eps*exp(logs)*ns)*mask");
  m.def("expand_states", &expand_states, "duration length-regulator gather");
  m.def("mask_tail_", &mask_tail_, "in-place zero of x[b,:,lens[b]:]");
  m.def("seeded_noise",
        [](long B, long C, long T, torch::Tensor lens, torch::Tensor seeds,
           const std::string& dt) {
          return seeded_noise(B, C, T, lens, seeds,
                              dt == "bf16" ? at::kBFloat16 : at::kFloat);
        },
        "per-utterance counter-based normal noise, one launch");
  m.def("row_ln_cl", &row_ln_cl,
        "LayerNorm over channel-last rows with fused residual add");
  m.def("depthwise_cl", &depthwise_cl, "channel-last depthwise conv1d");
  m.def("wn_step", &wn_step,
        "flow WaveNet residual/skip update in place (layer 0 first, 1 "
        "middle, 2 last); returns output",
        py::arg("h"), py::arg("output"), py::arg("rs"), py::arg("mc"),
        py::arg("layer"));
  m.def("flow_split_rev", &flow_split_rev,
        "xc [B,F,C] -> the (x0, x1) halves of flip(xc, -1)");
  m.def("coupling_tail", &coupling_tail,
        "coupling-flow tail fused with the next flow's flip; last: "
        "[cat(x0, x1_new)]",
        py::arg("x0"), py::arg("x1"), py::arg("post"), py::arg("mc"),
        py::arg("last"));
  m.def("dds_sep_ln_gelu", &dds_sep_ln_gelu,
        "DDS layer head: (x [+ g])*m -> depthwise k3 -> LN -> GELU; "
        "returns [y] or, with g, [y, x + g]",
        py::arg("x"), py::arg("g"), py::arg("mc"), py::arg("w"),
        py::arg("bias"), py::arg("gamma"), py::arg("beta"), py::arg("dil"),
        py::arg("eps") = 1e-5);
  m.def("ln_gelu_add", &ln_gelu_add,
        "DDS layer tail: t + GELU(LN(y)), times the mask when last",
        py::arg("y"), py::arg("t"), py::arg("mc"), py::arg("gamma"),
        py::arg("beta"), py::arg("last"), py::arg("eps") = 1e-5);
  m.def("rq_spline_inverse", &sonata::rq_spline_inverse,
        "dense, sync-free inverse rational-quadratic spline (no logabsdet); "
        "tail_kernel: the part after softmax/cumsum/softplus as one kernel",
        py::arg("inputs"), py::arg("uw"), py::arg("uh"), py::arg("ud"),
        py::arg("tail_bound") = 5.0, py::arg("tail_kernel") = false);
  m.def("spline_tail", &spline_tail,
        "per-element tail of the inverse spline on cumsum'd widths/heights "
        "and softplus'd derivatives",
        py::arg("inputs"), py::arg("cumwidths"), py::arg("cumheights"),
        py::arg("derivatives"), py::arg("tail_bound") = 5.0);
  m.def("prior_sample_rows", &prior_sample_rows,
        "prior_sample with noise_scale f32 [B] on the device, one per row",
        py::arg("m"), py::arg("logs"), py::arg("mask"), py::arg("noise"),
        py::arg("noise_scale"));
  m.def("scale_mask_rows", &scale_mask_rows,
        "z = noise * scales[b] * mask; scales f32 [B], product rounded once",
        py::arg("noise"), py::arg("mask"), py::arg("scales"));
  m.def("duration_rows", &duration_rows,
        "exp(logw)*x_mask*length_scale[b] -> ceil -> (durs int32 [B,T], "
        "y_lengths int64 [B]); bit-identical to the eager chain",
        py::arg("logw"), py::arg("x_mask"), py::arg("length_scale"));
  m.def("conv1d_fused", &conv1d_fused, "MFMA conv1d with fused activations");
  m.def("convtranspose1d_fused", &convtranspose1d_fused,
        "MFMA transposed conv1d (phase-decomposed GEMMs)");
  m.def("conv1d_cl_fused", &conv1d_cl_fused,
        "channel-last MFMA conv1d, fused act/residual/mask");
  m.def("convtranspose1d_cl_fused", &convtranspose1d_cl_fused,
        "channel-last MFMA transposed conv1d, phase-merged");
  m.def("conv1d_cl_wdirect", &conv1d_cl_wdirect,
        "hybrid: A staged in LDS, weights direct from L2 (no W barriers)");
  m.def("conv1d_direct_cl", &conv1d_direct_cl,
        "zero-LDS direct channel-last conv (L1/L2-fed MFMA)");
  m.def("resblock_pair_cl_fused", &resblock_pair_cl_fused,
        "fused HiFi-GAN resblock conv pair (xt stays in LDS)");
  m.def("resblock_wlayout_sliced", &resblock_wlayout_sliced,
        "does SONATA_RB_WLAYOUT (or the default) select sliced weights at CP");
  m.def("resblock_pair_cl_fused_sliced", &resblock_pair_cl_fused_sliced,
        "resblock conv pair, weights in the sliced [k][CP/32][CP][32] layout");
  m.def("resblock_chain_cl_fused", &resblock_chain_cl_fused,
        "whole resblock (3 pairs) fused: intermediates never touch HBM");
  m.def("attn_relpos_cl", &attn_relpos_cl,
        "fused relative-position attention (QKT+band+softmax+PV+rel_v)",
        py::arg("qkv"), py::arg("rel_k"), py::arg("rel_v"), py::arg("lens"),
        py::arg("heads"), py::arg("window"), py::arg("scale"));
  m.def("resample_linear_rows", &resample_linear_rows,
        "per-row linear resampling of [B,N] f32, positions in double");
  m.def("scale_rows", &scale_rows, "per-row gain of [B,N] f32");
  m.def("wsola_rows", &wsola_rows,
        "per-row WSOLA time stretch; returns (y, targets)",
        py::arg("x"), py::arg("in_len"), py::arg("ana_hop"),
        py::arg("n_frames"), py::arg("out_len"), py::arg("window"),
        py::arg("half"), py::arg("search"), py::arg("gain"),
        py::arg("n_out_max"), py::arg("k_max"));
  m.def("wsola_stream_rows", &wsola_stream_rows,
        "one round of per-row streaming WSOLA on carry ++ chunk; updates "
        "carry and tails in place, returns (y, targets)",
        py::arg("x"), py::arg("par"), py::arg("hop"), py::arg("gain"),
        py::arg("carry"), py::arg("tails"), py::arg("window"),
        py::arg("half"), py::arg("search"), py::arg("n_out"),
        py::arg("k_max"));
  m.def("resample_stream_rows", &resample_stream_rows,
        "one round of per-row streaming linear resampling on carry ++ "
        "chunk; updates carry in place, returns y",
        py::arg("x"), py::arg("par"), py::arg("carry"), py::arg("n_out"));
  m.def("pcm16_rows", &pcm16_rows,
        "per-row peak-normalised int16 PCM of [B,N] f32/bf16; returns "
        "(pcm [B,n_out], peaks)",
        py::arg("x"), py::arg("len"), py::arg("n_out"),
        py::arg("peak_normalize") = true);
  m.attr("PCM_TILE") = pcm_tile();
  m.def("g711_rows", &g711_rows,
        "per-row peak-normalised G.711 codes of [B,N] f32/bf16; law is "
        "int32 [B], 0 = mu-law, 1 = A-law; returns (codes uint8 [B,n_out], "
        "peaks)",
        py::arg("x"), py::arg("len"), py::arg("law"), py::arg("n_out"),
        py::arg("peak_normalize") = true);
  m.def("resample_poly_rows", &resample_poly_rows,
        "per-row polyphase FIR sample-rate conversion of [B,N] f32/bf16 by "
        "L/M; bank is the [K][L] f32 filter; returns y [B,n_out] f32",
        py::arg("x"), py::arg("in_len"), py::arg("out_len"), py::arg("bank"),
        py::arg("L"), py::arg("M"), py::arg("H"), py::arg("n_out"));
  m.def("resample_poly_stream_rows", &resample_poly_stream_rows,
        "one round of per-row streaming polyphase FIR conversion on carry "
        "++ chunk; state f32 [S,2,Kc] is ping-pong (reads buffer parity, "
        "writes the other); returns y [R,n_out] f32",
        py::arg("x"), py::arg("par"), py::arg("state"), py::arg("bank"),
        py::arg("L"), py::arg("M"), py::arg("H"), py::arg("n_out"));
  m.attr("RESAMPLE_TILE") = resample_tile();
  m.def("gather_windows", &gather_windows,
        "pack ragged latent windows of several [b,C,F] sources into "
        "[R,C,l_max], zero padded; one launch",
        py::arg("zs"), py::arg("src"), py::arg("row"), py::arg("start"),
        py::arg("length"), py::arg("l_max"));
  m.def("stream_seam_rows", &stream_seam_rows,
        "per-row trim + 42-sample crossfade of decoded stream chunks; "
        "writes tails_out at the named slots, returns out [R,n_out] f32",
        py::arg("wav"), py::arg("lo"), py::arg("hi"), py::arg("ext"),
        py::arg("prev_ext"), py::arg("slot"), py::arg("tails_in"),
        py::arg("tails_out"), py::arg("ramp"), py::arg("n_out"));
  m.attr("SEAM_CROSSFADE") = seam_crossfade_samples();

  // C++ inference runtime (csrc/engine): the ort-replacement executor.
  py::class_<sonata::VitsEngine>(m, "VitsEngine")
      .def(py::init([](const std::string& path, const std::string& device,
                       const std::string& dtype) {
             torch::Device dev(device);
             torch::Dtype dt =
                 dtype == "bf16" ? torch::kBFloat16 : torch::kFloat32;
             return new sonata::VitsEngine(path, dev, dt);
           }),
           py::arg("config_path"), py::arg("device") = "cpu",
           py::arg("dtype") = "f32")
      .def("infer",
           [](sonata::VitsEngine& e, torch::Tensor ids,
              torch::Tensor lengths, c10::optional<torch::Tensor> sid,
              double ns, double ls, double nw,
              std::vector<int64_t> seeds) {
             std::pair<torch::Tensor, torch::Tensor> r;
             {
               // release the GIL for the whole graph: concurrent server
               // handler threads serialize WAVs while the GPU runs
               py::gil_scoped_release rel;
               r = e.infer(ids, lengths, sid, ns, ls, nw, seeds);
             }
             return py::make_tuple(r.first, r.second);
           },
           py::arg("ids"), py::arg("lengths"),
           py::arg("sid") = py::none(), py::arg("noise_scale") = 0.667,
           py::arg("length_scale") = 1.0, py::arg("noise_w") = 0.8,
           py::arg("seeds") = std::vector<int64_t>{})
      .def("infer_encoder",
           [](sonata::VitsEngine& e, torch::Tensor ids,
              torch::Tensor lengths, c10::optional<torch::Tensor> sid,
              double ns, double ls, double nw,
              std::vector<int64_t> seeds) {
             std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> r;
             {
               py::gil_scoped_release rel;
               r = e.infer_encoder(ids, lengths, sid, ns, ls, nw, seeds);
             }
             return py::make_tuple(std::get<0>(r), std::get<1>(r),
                                   std::get<2>(r));
           },
           py::arg("ids"), py::arg("lengths"),
           py::arg("sid") = py::none(), py::arg("noise_scale") = 0.667,
           py::arg("length_scale") = 1.0, py::arg("noise_w") = 0.8,
           py::arg("seeds") = std::vector<int64_t>{})
      .def("infer_rows",
           [](sonata::VitsEngine& e, torch::Tensor ids,
              torch::Tensor lengths, c10::optional<torch::Tensor> sid,
              std::vector<double> ns, std::vector<double> ls,
              std::vector<double> nw, std::vector<int64_t> seeds) {
             std::pair<torch::Tensor, torch::Tensor> r;
             {
               py::gil_scoped_release rel;
               r = e.infer(ids, lengths, sid, ns, ls, nw, seeds);
             }
             return py::make_tuple(r.first, r.second);
           },
           py::arg("ids"), py::arg("lengths"), py::arg("sid"),
           py::arg("noise_scale"), py::arg("length_scale"),
           py::arg("noise_w"), py::arg("seeds") = std::vector<int64_t>{})
      .def("infer_encoder_rows",
           [](sonata::VitsEngine& e, torch::Tensor ids,
              torch::Tensor lengths, c10::optional<torch::Tensor> sid,
              std::vector<double> ns, std::vector<double> ls,
              std::vector<double> nw, std::vector<int64_t> seeds) {
             std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> r;
             {
               py::gil_scoped_release rel;
               r = e.infer_encoder(ids, lengths, sid, ns, ls, nw, seeds);
             }
             return py::make_tuple(std::get<0>(r), std::get<1>(r),
                                   std::get<2>(r));
           },
           py::arg("ids"), py::arg("lengths"), py::arg("sid"),
           py::arg("noise_scale"), py::arg("length_scale"),
           py::arg("noise_w"), py::arg("seeds") = std::vector<int64_t>{})
      .def("decode",
           [](sonata::VitsEngine& e, torch::Tensor z, torch::Tensor y_mask,
              c10::optional<torch::Tensor> g,
              c10::optional<torch::Tensor> lengths) {
             py::gil_scoped_release rel;
             return e.decode(z, y_mask, g, lengths);
           },
           py::arg("z"), py::arg("y_mask"), py::arg("g") = py::none(),
           py::arg("lengths") = py::none())
      .def("phonemes_to_ids", &sonata::VitsEngine::phonemes_to_ids)
      .def_property_readonly(
          "sample_rate",
          [](sonata::VitsEngine& e) { return e.config().sample_rate; })
      .def_property_readonly(
          "num_speakers",
          [](sonata::VitsEngine& e) { return e.config().num_speakers; })
      .def_property_readonly("hop", [](sonata::VitsEngine& e) {
        return e.config().hop();
      });
}
