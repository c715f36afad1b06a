"""What the CPU tests of the training loop (train.train) share: synthetic samples and the stand-ins for the HIP model and loss that
hooks["model_factory"] / hooks["criterion_factory"] take."""
import torch


def mix_sample(reads, seed):
    from gnnome_assembly_amd import synth, AssemblyGraph
    from gnnome_assembly_amd.train import GraphSample
    src, dst, n = synth.make_graph(reads, seed=seed)
    inp = synth.make_inputs(src, dst, n, seed=seed)
    return GraphSample(AssemblyGraph(src, dst, n), torch.from_numpy(inp["e"]), torch.from_numpy(inp["pe"]), torch.from_numpy(inp["y"]))


def oracle_model_factory(hp):
    """The package's own module class with its forward routed to the fp32 oracle."""
    import gnnome_assembly_amd as G
    from oracle import gatedgcn_oracle as orc

    class OracleModel(G.GraphGatedGCNModel):
        def forward(self, graph, x, e, pe):
            s, d = graph.edges()
            return orc.model_forward(dict(self.named_parameters()), s.long(), d.long(), graph.num_nodes(), e, pe)
    return OracleModel(hp["node_features"], hp["edge_features"], hp["dim_latent"], hp["hidden_edge_features"], hp["num_gnn_layers"],
                       hp["hidden_edge_scores"], hp["batch_norm"], hp["nb_pos_enc"])


class CountingBCE(torch.nn.BCEWithLogitsLoss):
    """torch's loss with the with_counts of the package's BCEWithLogitsLoss, in torch operations: the loop's fused-metrics route
    without a HIP device."""

    def with_counts(self, pred, y, acc=None):
        from gnnome_assembly_amd.train import tfpn_counts
        loss, counts = self(pred, y), tfpn_counts(pred.detach(), y)
        if acc is not None:
            acc.loss_sum += loss.detach().double()
            acc.steps += 1
            acc.counts += counts
        return loss, counts
